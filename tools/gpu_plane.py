"""Timing of PlaneEstimation (svh_plane_*): ms per call, with the phases of svh_plane_get_timing, for
    resident     one call on a device-resident 1242x375 map (urban2_stereomapper d1, seed 2)
    host         one call on the same map in host memory
    batch4/32    svh_plane_estimate_batch over 4 / 32 resident maps (the four urban maps, repeated)
    half         one call on the resident 621x187 map (urban4_kitti d1 decimated)
One JSON line per figure.

    python tools/gpu_plane.py [--calls N] [--warmup W]   on the GPU: every figure is a child process under its own
                                                         time limit, and the first one that fails ends the run
    python tools/gpu_plane.py --cpu-ref [--reps R]       the reference's call on one core, measured by
                                                         tests/plane/ref_plane_harness.cpp bench (needs the reference's
                                                         sources: build machine only)

Method: a host clock around the call, which ends in a stream wait; W warm-up calls thrown away (they load the kernels,
grow the buffers and fill the cache of raw draws), then N calls; median, min and p90."""
import argparse
import ctypes as C
import json
import os
import platform
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stereo-vision_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import plane_ref as R  # noqa: E402

FIGURES = ["resident", "host", "batch4", "batch32", "half"]
STEP_LIMIT_S = 150
PHASES = ["list_ms", "walk_ms", "vote_ms", "refit_ms", "call_ms", "list_device_ms", "vote_device_ms"]


def stats(ms):
    ms = np.sort(np.asarray(ms))
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(ms[0]), 4),
            "p90_ms": round(float(ms[int(0.9 * (len(ms) - 1))]), 4), "n": len(ms)}


def figure(name, calls, warmup):
    import svhip as S
    hip = C.CDLL("libamdhip64.so")

    def dev(a):
        p = C.c_void_p()
        a = np.ascontiguousarray(a)
        assert hip.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
        assert hip.hipMemcpy(p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0
        return p.value

    wall, phases = [], []
    if name in ("resident", "host", "half"):
        D = R.urban_d1("urban2_stereomapper") if name != "half" else R.half_map("urban4_kitti")
        h, w = D.shape
        pl = S.PlaneEstimation()
        pl.set_timing(True)
        addr = None if name == "host" else dev(D)
        for k in range(warmup + calls):
            t0 = time.perf_counter()
            rc = pl.estimate(D, seed=2) if addr is None else pl.estimate(addr, width=w, height=h, step=w, seed=2)
            t1 = time.perf_counter()
            assert rc == 0
            if k >= warmup:
                wall.append(1e3 * (t1 - t0))
                phases.append(pl.timing())
        n, size = 1, "%dx%d" % (w, h)
    else:
        n = int(name[5:])
        maps = [dev(R.urban_d1(u)) for u in R.URBAN]
        objs = [S.PlaneEstimation() for _ in range(n)]
        objs[0].set_timing(True)
        addrs = [maps[i % 4] for i in range(n)]
        seeds = [(0, 2, 12345)[(i // 4) % 3] for i in range(n)]
        for k in range(warmup + calls):
            t0 = time.perf_counter()
            st = S.PlaneEstimation.estimate_batch(objs, addrs, R.W, R.HGT, R.W, seeds=seeds)
            t1 = time.perf_counter()
            assert st == [0] * n
            if k >= warmup:
                wall.append(1e3 * (t1 - t0))
                phases.append(objs[0].timing())
        size = "%dx%d" % (R.W, R.HGT)
    out = {"figure": name, "maps": n, "size": size, "warmup": warmup, "version": S.lib().svh_version().decode()}
    out.update(stats(wall))
    med = np.median(np.asarray(phases), axis=0)
    out.update({k: round(float(v), 4) for k, v in zip(PHASES, med)})
    if n > 1:
        out["per_map_ms"] = round(out["median_ms"] / n, 4)
    print(json.dumps(out), flush=True)


def cpu_ref(reps):
    with tempfile.TemporaryDirectory() as tmp:
        exe = R.build_harness(tmp)
        for label, D, w in (("1242x375 urban2_stereomapper seed 2", R.urban_d1("urban2_stereomapper"), R.W),
                            ("1242x375 urban1_robotics seed 2", R.urban_d1("urban1_robotics"), R.W),
                            ("621x187 urban4_kitti decimated seed 2",
                             R.half_map("urban4_kitti"), 621)):
            text = R.run_bench(exe, tmp, [(D, w, 2)], reps)
            f = text.split()
            print(json.dumps({"figure": "reference", "map": label, "median_ms": float(f[3]), "min_ms": float(f[5]),
                              "max_ms": float(f[7]), "n": reps, "flags": " ".join(R.REFFLAGS),
                              "machine": "build machine, one core, %s" % platform.processor()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--cpu-ref", action="store_true")
    ap.add_argument("--figure")
    a = ap.parse_args()
    if a.cpu_ref:
        return cpu_ref(a.reps)
    if a.figure:
        return figure(a.figure, a.calls, a.warmup)
    for name in FIGURES:   # a fresh process per figure; the first failure ends the run
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--figure", name, "--calls", str(a.calls),
                             "--warmup", str(a.warmup)], timeout=STEP_LIMIT_S).returncode
        if rc != 0:
            print(json.dumps({"figure": name, "failed": rc}), flush=True)
            sys.exit(1)


if __name__ == "__main__":
    main()
