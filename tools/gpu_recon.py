"""Timing of Reconstruction::update (svh_recon_*): ms per update on the `synth` and `frames` scenes of
tests/golden/recon.npz, split by svh_recon_get_timing into host bookkeeping, device time (uploads + k_recon_tracks +
k_recon_compact, HIP events) and the copy-back of the outcomes, and the same with the lost tracks handed to the lanes
sorted by length (SVH_RECON_SORT=1).  One JSON line per figure.

    python tools/gpu_recon.py [--reps R]            on the GPU: every step is a child process under its own time
                                                    limit, and the first one that fails ends the run
    python tools/gpu_recon.py --cpu-ref [--reps R]  the reference's update() on one core, measured the same way by
                                                    tests/recon/ref_recon_harness.cpp bench (needs the reference's
                                                    sources: build machine only)

Method: a host clock around update(), which ends in a stream wait.  A fresh object per repetition, every update of
the scene timed, repetition 0 thrown away (it loads the kernels and grows the buffers)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stereo-vision_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import recon_ref as R  # noqa: E402

RUNS = [("synth", 1), ("frames", 0)]   # (scene, index of the setting): update(.., 1, 2, 30, 2) on both
STEP_LIMIT_S = 120


def stats(ms):
    ms = np.sort(np.asarray(ms))
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(ms[0]), 4),
            "p90_ms": round(float(ms[int(0.9 * (len(ms) - 1))]), 4), "n": len(ms)}


def load():
    with np.load(R.GOLDEN) as z:
        return {k: z[k] for k in z.files}


def step(name, j, reps):
    import svhip as S
    Z = load()
    scene = [(Tr, R.to_p_match(m)) for Tr, m in R.unpack_scene(Z, name)]
    s = Z["%s_settings" % name][j]
    calib = [float(c) for c in Z["calib"]]
    wall, split, lost = [], [], []
    for r in range(reps + 1):
        rec = S.Reconstruction()
        rec.set_calibration(*calib)
        rec.set_timing(True)
        for Tr, m in scene:
            t0 = time.perf_counter()
            rec.update(m, Tr, int(s[0]), int(s[1]), float(s[2]), float(s[3]))
            ms = 1e3 * (time.perf_counter() - t0)
            if r:
                wall.append(ms)
                split.append(rec.timing())
                lost.append(len(rec.outcomes()[0]))
        points = rec.num_points()
        rec.close()
    assert points == len(Z["%s_%d_points" % (name, j)])
    sp = np.median(np.array(split), axis=0)
    print(json.dumps(dict(figure="gpu_update", scene=name, setting=[float(x) for x in s],
                          sorted_by_length=os.environ.get("SVH_RECON_SORT", "0"), updates=len(scene),
                          lost_per_update_median=int(np.median(lost)), lost_per_update_max=int(max(lost)),
                          host_ms=round(float(sp[0]), 4), device_ms=round(float(sp[1]), 4),
                          copy_back_ms=round(float(sp[2]), 4), points=points, **stats(wall))), flush=True)


def gpu(reps):
    for sort in ("0", "1"):
        for name, j in RUNS:
            env = dict(os.environ, SVH_RECON_SORT=sort)
            rc = subprocess.call(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__),
                                  "--step", name, str(j), "--reps", str(reps)], env=env)
            if rc != 0:
                print(json.dumps(dict(figure="gpu_update", scene=name, failed=rc)), flush=True)
                return rc
    return 0


def cpu_ref(reps):
    Z = load()
    with tempfile.TemporaryDirectory() as tmp:
        exe = R.build_harness(tmp)
        for name, j in RUNS:
            scene = R.unpack_scene(Z, name)
            path = os.path.join(tmp, name + ".bin")
            R.write_scene(path, scene)
            txt = R.run_bench(exe, path, Z["%s_settings" % name][j], reps, tuple(Z["calib"])).split()
            print(json.dumps(dict(figure="cpu_ref_update", scene=name, median_ms=float(txt[1]), mean_ms=float(txt[3]),
                                  max_ms=float(txt[5]), updates=int(txt[7]), points=int(txt[9]))), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-ref", action="store_true")
    ap.add_argument("--step", nargs=2)
    a = ap.parse_args()
    if a.step:
        step(a.step[0], int(a.step[1]), a.reps)
        return 0
    return cpu_ref(a.reps) if a.cpu_ref else gpu(a.reps)


if __name__ == "__main__":
    sys.exit(main())
