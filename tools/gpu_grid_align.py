#!/usr/bin/env python3
"""Time the alignment of a frame to the local grid (svh_grid_align_points, include/svh_grid.h, "ALIGN") on the device.

Scenes: windows of 256 x 256 and 1024 x 1024 cells of 0.2 m (min_points 1), one cell in eight an obstacle, the pivot in the middle,
reach 0.6 m, range 25.6 m (the box of the scan is 1025 x 1025 subs).  The frame is n_scan distinct subs drawn from the obstacle cells
inside the box, moved by (3, -2) subs, two points per sub, resident on the device.  n_scan = 10^3, 10^4, 10^5; (K, W) = (8, 8) and
(32, 32): 4 913 and 274 625 candidates.

One repetition of a side is timed with the host clock around whole calls, which return after their last stream wait:
  device        svh_grid_align_points on the device-resident points with the field cached: marks, compaction, scores, best, the
                record's copy
  device_plain, device_tiled  the same with the other two forms of the score kernel (svh_test_grid_align_form): one lane per
                candidate over the whole scan with F from global memory; F staged in LDS with the translations a whole cell apart
                sharing their weights.  `device` is the chunk form
  device_stale  svh_grid_add_points of one host point first (its copy and binning; every cached plane is stale), then the same: the
                finished planes and the field are computed again -- what a caller pays per frame
  device_stale_mask  the same with the field in three launches, as the cost layer's -- a mask from STATE, the column sweep, the row
                pass -- instead of the two kept, whose column sweep reads STATE in place
  host          what a caller does without it: STATE to the host (svh_grid_get_local) and the header's host form there
                (svh_test_grid_align: field, scan, align_window) on a host copy of the points.  Not run where candidates x n_scan
                exceeds 10^9 (a repetition would take minutes); such a line has no host numbers
The sides alternate repetition by repetition in one process, the order reversed every other time.  Before anything is timed the
record, the scan and the volume of the device are compared with the host's (where the host runs).  Per case 3 warm-up and 20 timed
repetitions (1 and 5 where a repetition takes more than a second): median, 10th and 90th percentile in ms, and the paired
difference host - device.  One JSON line per case goes to profiles/grid_align_times.jsonl.  There is no threshold: this is a
measurement.

    python tools/gpu_grid_align.py [--out FILE] [--sizes 256,1024] [--scans 1000,10000,100000] [--windows 8x8,32x32]
                                   [--reps WARMUP,TIMED] [--tag TEXT]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stereo-vision_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gpu_grid_plan import CELL, paired, summary   # noqa: E402

HOST_LIMIT = 10 ** 9


def main():
    out = os.path.join(ROOT, "profiles", "grid_align_times.jsonl")
    sizes, scans, windows, warmup, timed, tag = [256, 1024], [1000, 10000, 100000], [(8, 8), (32, 32)], 3, 20, ""
    argv = sys.argv[1:]
    try:
        while argv:
            flag, value = argv[0], argv[1]
            argv = argv[2:]
            if flag == "--out":
                out = value
            elif flag == "--sizes":
                sizes = [int(v) for v in value.split(",")]
            elif flag == "--scans":
                scans = [int(v) for v in value.split(",")]
            elif flag == "--windows":
                windows = [tuple(int(x) for x in v.split("x")) for v in value.split(",")]
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
    hip = C.CDLL("libamdhip64.so")
    frame = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0]], np.float64)
    lines = []

    def emit(rec):
        rec = dict(dict(version=svhip.lib().svh_version().decode(), tag=tag), **rec)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for n in sizes:
        rng = np.random.default_rng(n)
        g = G.Grid(G.default_params(nx=n, nz=n, cell=CELL, x0=0.0, z0=0.0, T=frame, min_points=1, step=0.2, clearance=2.0))
        wall = rng.random((n, n)) < 0.125
        b, a = np.nonzero(np.ones((n, n), bool))
        pts = np.zeros((n * n, 4), np.float32)
        pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3] = (a + 0.5) * CELL, np.where(wall.ravel(), -1.0, 0.0), (b + 0.5) * CELL, 0.5
        g.add_points(pts)
        one = np.array([[0.5 * CELL, 0.0, 0.5 * CELL, 0.5]], np.float32)                      # a second ground point on a corner cell
        pivot = np.array([n / 2 * CELL + 0.01, 0.0, n / 2 * CELL + 0.01], np.float64)
        Pa = Pb = 4 * (n // 2)
        wb, wa = np.nonzero(wall)
        inside = (np.abs(4 * wa - Pa) < 500) & (np.abs(4 * wb - Pb) < 500)
        wa, wb = wa[inside], wb[inside]
        i, j = (v.ravel() for v in np.meshgrid(np.arange(4), np.arange(4)))
        every = np.stack([(4 * wa[:, None] + i[None, :]).ravel(), (4 * wb[:, None] + j[None, :]).ravel()], 1)      # the 16 subs of every obstacle cell
        for n_scan in scans:
            assert len(every) >= n_scan, (n, n_scan, len(every))
            subs = every[rng.choice(len(every), n_scan, replace=False)] + np.array([3, -2])
            fp = np.zeros((2 * n_scan, 4), np.float32)
            fp[:, 0], fp[:, 2] = np.tile((subs[:, 0] + 0.5) * CELL / 4, 2), np.tile((subs[:, 1] + 0.5) * CELL / 4, 2)
            fp[:, 1], fp[:, 3] = np.repeat([-1.0, -1.5], n_scan), 0.5
            fp = fp[rng.permutation(len(fp))]
            d = C.c_void_p()
            assert hip.hipMalloc(C.byref(d), C.c_size_t(fp.nbytes)) == 0
            assert hip.hipMemcpy(d, C.c_void_p(fp.ctypes.data), C.c_size_t(fp.nbytes), 1) == 0
            for K, W in windows:
                g.set_align(reach=0.6, range=25.6, rot_den=256, rot_n=K, trans_n=W, min_scan=32)
                cands = (2 * K + 1) * (2 * W + 1) ** 2
                with_host = cands * n_scan <= HOST_LIMIT
                got = {}

                def device(form=0, key="rec"):
                    G.align_form(form)
                    t0 = time.perf_counter()
                    got[key] = g.align_points_device(d.value, len(fp), pivot)
                    t = (time.perf_counter() - t0) * 1e3
                    G.align_form(0)
                    return t

                def device_stale(form=0):
                    G.align_form(form)
                    t0 = time.perf_counter()
                    g.add_points(one)
                    got["rec"] = g.align_points_device(d.value, len(fp), pivot)
                    t = (time.perf_counter() - t0) * 1e3
                    G.align_form(0)
                    return t

                def host():
                    t0 = time.perf_counter()
                    got["host"] = G.core_align(g.params, g.align_params, g.local_plane(G.LOCAL_STATE), 0, 0, points=fp, pivot=pivot)
                    return (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                device_stale()
                slow = time.perf_counter() - t0 > 1.0
                assert got["rec"][0] == G.ALIGN_OK and got["rec"][6] == n_scan, got["rec"]
                sides = {"device": device, "device_plain": lambda: device(1, "plain"), "device_tiled": lambda: device(2, "tiled"), "device_stale": device_stale,
                         "device_stale_mask": lambda: device_stale(4)}
                volumes = []
                for form in range(3):                                                     # the three forms give the same bytes
                    device(form)
                    volumes.append(g.align_volume().tobytes())
                assert volumes[0] == volumes[1] == volumes[2], (n, n_scan, K, W)
                if with_host:
                    t0 = time.perf_counter()
                    host()
                    slow = slow or time.perf_counter() - t0 > 1.0
                    h = got["host"]
                    assert np.array_equal(h["rec"], got["rec"]) and np.array_equal(h["scan"], g.align_scan()) and np.array_equal(h["volume"], g.align_volume()), (n, n_scan, K, W)
                    sides["host"] = host
                ms = paired(sides, 1 if slow else warmup, 5 if slow else timed)
                rec = dict(case="align_points", size=n, n_scan=n_scan, points=len(fp), K=K, W=W, candidates=cands, record=[int(v) for v in got["rec"]],
                           host_measured=with_host, reps=len(ms["device"]))
                for name, v in ms.items():
                    rec.update(summary(name, v))
                rec.update(summary("mask_minus_stale", [x - y for x, y in zip(ms["device_stale_mask"], ms["device_stale"])]))
                rec.update(summary("plain_minus_device", [x - y for x, y in zip(ms["device_plain"], ms["device"])]))
                rec.update(summary("tiled_minus_device", [x - y for x, y in zip(ms["device_tiled"], ms["device"])]))
                if with_host:
                    rec.update(summary("host_minus_device", [x - y for x, y in zip(ms["host"], ms["device"])]))
                emit(rec)
            hip.hipFree(d)
        g.close()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
