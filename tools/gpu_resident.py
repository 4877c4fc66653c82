"""What the device-frame entries are worth per frame: tools/stereomapper_pipeline.py's Pipeline with and without
`resident`, on the same seeded drive, in one process.

    python tools/gpu_resident.py [--frames 40] [--warmup 5] [--reps 3] [--out profiles/resident_frames_times.jsonl]

Two inputs, each 40 frames of one synthetic scene that moves two pixels a frame (tests/helpers.py synth_pair):
    raw        1392 x 512 frames, rectified on the device to 1242 x 375 with the rig calibration of
               tests/golden/rectify.npz (Pipeline(rectify_params=...), the tool's --unrectified)
    rectified  1242 x 375 frames
Per input the two variants alternate frame by frame (which of them goes first alternates too), each on its own
Pipeline and with a private random stream, so both see every frame under the same conditions.  The first --warmup frames
of each are not timed.  The drive is run --reps times, with fresh Pipelines each time, and the per-frame times are
pooled.  Method: a host clock around whole Pipeline.push calls; every push ends in the library's own waits (the map
fusion's stream wait is its last device step).  The results of the two variants (ok flag and both point-list counts per
frame) must be equal, or the tool stops.

One JSON line per input and variant: median, min, 10th and 90th percentile of the per-frame time in ms, and for the
resident variant the median of the per-frame differences (host_hop - resident), which the alternation makes a paired
comparison.  The file is rewritten by every run."""
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

CALIB = (645.24, 635.96, 194.13, 0.5707)     # libviso2 demo.cpp, what the pipeline test uses
RIG_SRC, RIG_DST = (1392, 512), (1242, 375)
STEP = 2                                     # pixels the scene moves per frame


def drive(size, frames, seed):
    import helpers as H
    w, h = size
    l, r = H.synth_pair(w + STEP * frames, h, seed)
    return [(np.ascontiguousarray(l[:, STEP * k:STEP * k + w]), np.ascontiguousarray(r[:, STEP * k:STEP * k + w]))
            for k in range(frames)]


def rig_params():
    """the two cameras of tests/golden/rectify.npz: K (9), D (5), R (9), P (12) each"""
    from svhip import rectify
    with np.load(os.path.join(ROOT, "tests", "golden", "rectify.npz")) as z:
        cams = []
        for c in range(2):
            v = z["rig%d_cam" % c]
            cams.append({"K": v[0:9], "D": v[9:14], "R": v[14:23], "P": v[23:35]})
    return rectify.params(RIG_SRC, RIG_DST, cams)


def stats(ms):
    ms = np.sort(np.asarray(ms, np.float64))
    q = lambda f: round(float(ms[int(f * (len(ms) - 1))]), 4)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": q(0), "p10_ms": q(0.1), "p90_ms": q(0.9), "n": len(ms)}


def measure(name, frames, warmup, reps, make):
    import svhip
    assert svhip.device_count() > 0, "no HIP device: nothing is measured without one"
    times = {"host_hop": [], "resident": []}
    oks = 0
    for rep in range(reps):
        pipes = {"host_hop": make(False), "resident": make(True)}
        for p in pipes.values():
            p.vo.lib.svh_vo_set_private_rand.argtypes = [C.c_void_p, C.c_int32, C.c_uint32]
            p.vo.lib.svh_vo_set_private_rand(p.vo.h, 1, 0)
        for k, (l, r) in enumerate(frames):
            order = ("host_hop", "resident") if (k + rep) % 2 == 0 else ("resident", "host_hop")
            res, ms = {}, {}
            for v in order:
                t0 = time.perf_counter()
                res[v] = pipes[v].push(l, r)
                ms[v] = (time.perf_counter() - t0) * 1e3
            if res["host_hop"] != res["resident"]:
                raise SystemExit("%s frame %d: the variants differ: %r vs %r" % (name, k, res["host_hop"], res["resident"]))
            if k >= warmup:
                for v in order:
                    times[v].append(ms[v])
            oks += int(res["resident"][0])
        del pipes
    lines = []
    for v in ("host_hop", "resident"):
        line = {"tool": "gpu_resident", "input": name, "variant": v, "frames_timed": len(times[v]),
                "frames": len(frames), "warmup": warmup, "reps": reps, "vo_ok": oks}
        line.update(stats(times[v]))
        if v == "resident":
            d = np.asarray(times["host_hop"]) - np.asarray(times["resident"])
            line["paired_saving_ms"] = {"median": round(float(np.median(d)), 4),
                                        "p10": round(float(np.sort(d)[int(0.1 * (len(d) - 1))]), 4),
                                        "p90": round(float(np.sort(d)[int(0.9 * (len(d) - 1))]), 4)}
        lines.append(line)
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resident_frames_times.jsonl"))
    a = ap.parse_args()
    if a.warmup >= a.frames:
        raise SystemExit("--warmup must be below --frames")
    import stereomapper_pipeline as SP
    lines = measure("raw 1392x512 -> 1242x375", drive(RIG_SRC, a.frames, 11), a.warmup, a.reps,
                    lambda res: SP.Pipeline(*CALIB, rectify_params=rig_params(), resident=res))
    lines += measure("rectified 1242x375", drive(RIG_DST, a.frames, 12), a.warmup, a.reps,
                     lambda res: SP.Pipeline(*CALIB, resident=res))
    with open(a.out, "w") as f:
        for line in lines:
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
