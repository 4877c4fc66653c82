"""What lockstep is worth per frame-step of K drives: tools/stereomapper_pipeline.py's LockstepPipeline (one
svh_vo_process_batch_device, svh_vo_get_gain_batch, svh_elas_process_batch_device and svh_map_add_batch_device per step)
against a loop of K single resident pushes (K Pipeline(resident=True)), on the same seeded drives, in one process.

    python tools/gpu_lockstep_chain.py [--frames 30] [--warmup 5] [--reps 2] [--K 1,4,16]
                                       [--out profiles/lockstep_chain_times.jsonl]

The K drives are 1242 x 375 crops of one synthetic scene that moves two pixels a frame (tests/helpers.py synth_pair),
drive i starting i frames in, so the drives differ.  Per K the two variants alternate step by step (which of them goes
first alternates too), each on its own objects and with private random streams, so both see every step under the same
conditions.  The first --warmup steps are not timed.  The drives are run --reps times, with fresh objects each time, and
the per-step times are pooled.  Method: a host clock around a whole step of K frames; every step ends in the library's
own waits (the views' accumulation follows the map fusion's stream wait).  The results of the two variants (ok flag and
both point-list counts per drive and step) must be equal, or the tool stops.

One JSON line per K and variant: median, min, 10th and 90th percentile of the per-step time in ms, the same per frame
(divided by K), and for the lockstep variant the median and the 10th / 90th percentile of the per-step differences
(loop - lockstep), which the alternation makes a paired comparison.  The file is rewritten by every run."""
import argparse
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
SIZE = (1242, 375)
STEP = 2                                     # pixels the scene moves per frame


def drives(K, frames, seed):
    import helpers as H
    w, h = SIZE
    l, r = H.synth_pair(w + STEP * (frames + K), h, seed)
    cut = lambda a, k: np.ascontiguousarray(a[:, STEP * k:STEP * k + w])
    return [[(cut(l, i + k), cut(r, i + k)) for k in range(frames)] for i in range(K)]


def stats(ms):
    ms = np.sort(np.asarray(ms, np.float64))
    q = lambda f: round(float(ms[int(f * (len(ms) - 1))]), 4)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": q(0), "p10_ms": q(0.1), "p90_ms": q(0.9), "n": len(ms)}


def measure(K, frames, warmup, reps, seed):
    import stereomapper_pipeline as SP
    import svhip
    assert svhip.device_count() > 0, "no HIP device: nothing is measured without one"
    seqs = drives(K, frames, seed)
    times = {"loop": [], "lockstep": []}
    oks = 0
    for rep in range(reps):
        lock = SP.LockstepPipeline(K, *CALIB, private_rand=0)
        loop = [SP.Pipeline(*CALIB, resident=True) for _ in range(K)]
        for p in loop:
            p.vo.lib.svh_vo_set_private_rand.argtypes = [SP.C.c_void_p, SP.C.c_int32, SP.C.c_uint32]
            p.vo.lib.svh_vo_set_private_rand(p.vo.h, 1, 0)
        run = {"lockstep": lambda pairs: [tuple(x) for x in lock.push(pairs)],
               "loop": lambda pairs: [tuple(p.push(l, r)) for p, (l, r) in zip(loop, pairs)]}
        for k in range(frames):
            pairs = [s[k] for s in seqs]
            order = ("loop", "lockstep") if (k + rep) % 2 == 0 else ("lockstep", "loop")
            res, ms = {}, {}
            for v in order:
                t0 = time.perf_counter()
                res[v] = run[v](pairs)
                ms[v] = (time.perf_counter() - t0) * 1e3
            if res["loop"] != res["lockstep"]:
                raise SystemExit("K = %d step %d: the variants differ: %r vs %r" % (K, k, res["loop"], res["lockstep"]))
            if k >= warmup:
                for v in order:
                    times[v].append(ms[v])
            oks += sum(int(x[0]) for x in res["lockstep"])
        del lock, loop, run
    lines = []
    for v in ("loop", "lockstep"):
        line = {"tool": "gpu_lockstep_chain", "input": "rectified %dx%d" % SIZE, "K": K, "variant": v,
                "steps_timed": len(times[v]), "steps": frames, "warmup": warmup, "reps": reps, "vo_ok": oks}
        line.update(stats(times[v]))
        line["per_frame_median_ms"] = round(line["median_ms"] / K, 4)
        if v == "lockstep":
            d = np.sort(np.asarray(times["loop"]) - np.asarray(times["lockstep"]))
            line["paired_saving_ms"] = {"median": round(float(np.median(d)), 4),
                                        "p10": round(float(d[int(0.1 * (len(d) - 1))]), 4),
                                        "p90": round(float(d[int(0.9 * (len(d) - 1))]), 4)}
        lines.append(line)
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--K", default="1,4,16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lockstep_chain_times.jsonl"))
    a = ap.parse_args()
    if a.warmup >= a.frames:
        raise SystemExit("--warmup must be below --frames")
    lines = []
    for K in (int(v) for v in a.K.split(",")):
        lines += measure(K, a.frames, a.warmup, a.reps, 30 + K)
        for line in lines[-2:]:
            print(json.dumps(line), flush=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
