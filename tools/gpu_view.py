#!/usr/bin/env python3
"""Time the render of the map view (include/svh_view.h) on the device.

Cases: N = 10^5, 10^6, 10^7 synthetic points, and the fused lists of the golden urban crops (urban2 and urban3
through svh_map_add, accumulated with svh_view_add_map), each at 1242 x 375 and at 320 x 480.  Per case 5 warm-up and
20 timed renders into a device buffer (no copy back), each bracketed by two HIP events on the stream hipEventRecord is
given -- the object's own stream is not exposed, so the events go to the null stream and a device synchronisation
orders them around the call; the event interval therefore contains the whole call on the device: the upload of the
segment list, the two clears, the three kernels.  Reported: median, minimum, maximum in ms and the bytes of the point
store streamed per second at the median.  One JSON line per case is appended to profiles/view_render_times.jsonl.

    python tools/gpu_view.py [--out FILE] [--max-points N]

There is no threshold: this is a measurement."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stereo-vision_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARMUP, TIMED = 5, 20
SIZES = [(1242, 375), (320, 480)]


class Timer:
    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.a, self.b = C.c_void_p(), C.c_void_p()
        assert self.hip.hipEventCreate(C.byref(self.a)) == 0 and self.hip.hipEventCreate(C.byref(self.b)) == 0

    def ms(self, call):
        hip = self.hip
        assert hip.hipDeviceSynchronize() == 0
        assert hip.hipEventRecord(self.a, None) == 0
        call()
        assert hip.hipEventRecord(self.b, None) == 0
        assert hip.hipEventSynchronize(self.b) == 0
        out = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(out), self.a, self.b) == 0
        return float(out.value)

    def malloc(self, nbytes):
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
        return p


def synthetic(n, seed=1):
    """a corridor of points in front of the first camera, like a drive's map"""
    rng = np.random.default_rng(seed)
    pts = np.empty((n, 4), np.float32)
    pts[:, 0] = rng.uniform(-8, 8, n)
    pts[:, 1] = rng.uniform(-2, 2, n)
    pts[:, 2] = rng.uniform(1, 120, n)
    pts[:, 3] = rng.uniform(0, 1, n)
    return pts


def urban_view(view_mod, size):
    import helpers as H
    from svhip import mapper
    m = mapper.Mapper(721.5377, 609.5593, 172.854, 0.5371657, 20.0)
    v = view_mod.View(*size)
    for k, name in enumerate(("urban2", "urban3")):
        z = np.load(os.path.join(H.GOLDEN, name + "_kitti.npz"))
        l, _ = H.golden_pair(str(z["crop"]))
        Ht = np.eye(4)
        Ht[2, 3] = 0.3 * k
        m.add(z["d1"].reshape(l.shape), l, Ht, 0.0)
        v.add_camera(Ht, 0.1, True)
        v.add_map(m)
    return v


def measure(timer, v, rgb):
    for _ in range(WARMUP):
        v.render(device_ptr=rgb.value)
    return sorted(timer.ms(lambda: v.render(device_ptr=rgb.value)) for _ in range(TIMED))


def main():
    import svhip
    from svhip import view
    out = os.path.join(ROOT, "profiles", "view_render_times.jsonl")
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
        raise SystemExit("gpu_view needs a GPU: libsvhip has no CPU fallback")
    timer = Timer()
    rgb = timer.malloc(1242 * 480 * 3)
    build = svhip.lib().svh_version().decode()
    lines = []
    for W, Hh in SIZES:
        cases = [("synthetic_%d" % n, n) for n in (10 ** 5, 10 ** 6, 10 ** 7) if n <= max_points] + [("urban2_urban3_fused", None)]
        for name, n in cases:
            if n is None:
                v = urban_view(view, (W, Hh))
            else:
                v = view.View(W, Hh)
                v.add_points([synthetic(n)])
            ms = measure(timer, v, rgb)
            med = 0.5 * (ms[TIMED // 2 - 1] + ms[TIMED // 2])
            npts = v.count(view.POINTS)
            rec = {"case": name, "width": W, "height": Hh, "points": npts, "cameras": v.count(view.CAMERAS),
                   "warmup": WARMUP, "timed": TIMED, "median_ms": round(med, 4), "min_ms": round(ms[0], 4),
                   "max_ms": round(ms[-1], 4), "store_gb_per_s": round(npts * 16 / (med * 1e-3) / 1e9, 2),
                   "timed_with": "HIP events around svh_view_render, device output", "build": build}
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
            v.close()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
