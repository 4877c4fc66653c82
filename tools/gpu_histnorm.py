"""What the histogram normalisation on the device costs (include/svh_histnorm.h): whole calls on device-resident pairs,
and a pipeline frame with and without it.

    python tools/gpu_histnorm.py [--calls 20] [--frames 24] [--warmup 4] [--reps 2] [--out profiles/histnorm_times.jsonl]

1. svh_histnorm_pairs_device on n = 1 and n = 32 pairs of 1242 x 375 and 1392 x 512 images that lie in device memory
   (a fixed pattern, every image different; uploaded again before every call, outside the clock, because the call
   works in place).  Method: a host clock around the whole call, which ends in the library's own stream wait; three
   untimed calls first, then the median, 10th and 90th percentile of --calls calls.  Next to it the device time of the
   same calls from the library's events (svh_histnorm_get_timing), and the byte model: per image N bytes read by
   k_hist_count, N read and N written by k_hist_apply, 3 N in all; `model_gbps` is that over the median call.
2. tools/stereomapper_pipeline.py's resident Pipeline with and without `normalize` on one synthetic drive (the scene of
   tools/gpu_resident.py), alternating frame by frame in one process, which of them goes first alternating too, each
   with a private random stream; a host clock around whole push calls.  The two variants see different pixels, so
   their results differ and the difference of their frame times is not the cost of the equalisation alone: ELAS and
   the matcher work on other images.  It is reported as measured, paired per frame, with its 10th and 90th percentile.

One JSON line per measurement; the file is rewritten by every run."""
import argparse
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

SIZES = ((1242, 375), (1392, 512))
PAIRS = (1, 32)


def images(w, h, n):
    """n different images: an integer hash of (u, v, k), squared so that the histogram is uneven"""
    v, u = np.mgrid[0:h, 0:w].astype(np.int64)
    out = np.empty((n, h, w), np.uint8)
    for k in range(n):
        x = (u * 7919 + v * 104729 + (u * v) % 8191 * 31 * (k + 1)) % 1000
        out[k] = (x * x) // (3922 + 40 * k)
    return out


def measure_calls(calls):
    import stereomapper_pipeline as SP
    from gpu_resident import stats
    from svhip import histnorm
    lines = []
    for w, h in SIZES:
        for n in PAIRS:
            N = w * h
            left, right = images(w, h, n), images(w, h, n)[::-1].copy()
            d1, d2 = SP.DeviceBuffer(n * N), SP.DeviceBuffer(n * N)
            o = histnorm.HistNorm(w, h)
            o.set_timing(True)
            host, dev = [], []
            for k in range(calls + 3):
                d1.upload(left)
                d2.upload(right)
                t0 = time.perf_counter()
                o.pairs_device(n, d1.ptr.value, d2.ptr.value, w, N)
                ms = (time.perf_counter() - t0) * 1e3
                if k >= 3:
                    host.append(ms)
                    dev.append(o.timing().copy())
            dev = np.median(np.asarray(dev), axis=0)
            line = {"tool": "gpu_histnorm", "what": "svh_histnorm_pairs_device, whole call, device-resident",
                    "width": w, "height": h, "pairs": n, "calls": calls, "model_bytes": 3 * N * 2 * n,
                    "device_ms_median": {"call": round(float(dev[0]), 4), "count_and_table": round(float(dev[1]), 4),
                                         "apply": round(float(dev[2]), 4)}}
            line.update(stats(host))
            line["model_gbps"] = round(3 * N * 2 * n / (line["median_ms"] * 1e-3) / 1e9, 2)
            lines.append(line)
            o.close()
    return lines


def measure_pipeline(frames, warmup, reps):
    import stereomapper_pipeline as SP
    from gpu_resident import CALIB, RIG_DST, drive, stats
    seq = drive(RIG_DST, frames, 12)
    times = {"plain": [], "normalize": []}
    for rep in range(reps):
        pipes = {"plain": SP.Pipeline(*CALIB, resident=True), "normalize": SP.Pipeline(*CALIB, resident=True, normalize=True)}
        for p in pipes.values():
            p.vo.lib.svh_vo_set_private_rand.argtypes = [C.c_void_p, C.c_int32, C.c_uint32]
            p.vo.lib.svh_vo_set_private_rand(p.vo.h, 1, 0)
        for k, (l, r) in enumerate(seq):
            order = ("plain", "normalize") if (k + rep) % 2 == 0 else ("normalize", "plain")
            ms = {}
            for v in order:
                t0 = time.perf_counter()
                pipes[v].push(l, r)
                ms[v] = (time.perf_counter() - t0) * 1e3
            if k >= warmup:
                for v in order:
                    times[v].append(ms[v])
        del pipes
    lines = []
    for v in ("plain", "normalize"):
        line = {"tool": "gpu_histnorm", "what": "resident Pipeline.push, whole frame", "input": "rectified 1242x375",
                "variant": v, "frames": frames, "warmup": warmup, "reps": reps}
        line.update(stats(times[v]))
        if v == "normalize":
            d = np.sort(np.asarray(times["normalize"]) - np.asarray(times["plain"]))
            line["paired_extra_ms"] = {"median": round(float(np.median(d)), 4), "p10": round(float(d[int(0.1 * (len(d) - 1))]), 4),
                                       "p90": round(float(d[int(0.9 * (len(d) - 1))]), 4)}
        lines.append(line)
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "histnorm_times.jsonl"))
    a = ap.parse_args()
    if a.warmup >= a.frames:
        raise SystemExit("--warmup must be below --frames")
    import svhip
    assert svhip.device_count() > 0, "no HIP device: nothing is measured without one"
    lines = measure_calls(a.calls) + measure_pipeline(a.frames, a.warmup, a.reps)
    with open(a.out, "w") as f:
        for line in lines:
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
