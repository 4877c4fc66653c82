"""Timing of VisualOdometryMono (svh_vo_mono_*): ms per process() over the reference's seven mono frames, ms per
estimate-only call (VisualOdometry::process(p_matched)) at N = 350 and N = 2000, and the device time of the
estimate's three phases from HIP events (RANSAC: k_mono_hyp + k_mono_vote + k_mono_select; chirality:
k_mono_chiral + k_mono_pick; plane vote: k_mono_plane; each with its upload).  One JSON line per figure.

    python tools/gpu_mono_vo.py [--reps R]            on the GPU
    python tools/gpu_mono_vo.py --cpu-ref [--reps R]  the reference on the CPU, measured the same way (needs the
                                                      reference's sources: build machine only)

Method: a host clock around calls that end in a device synchronise.  process(): a fresh object per repetition
(outside the clock), frames 0-6 in order, frames 1-6 timed (frame 0 only fills the ring buffer), the calibration
of demo_viso_mono.m with motion_threshold 1e6 so that every estimate runs to the end.  Estimate-only: the seeded
synthetic scenes of tests/mono_ref.py (20 % outliers), one object, R calls after one untimed call."""
import argparse
import json
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stereo-vision_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers as H  # noqa: E402
import mono_ref as R  # noqa: E402

P = dict(R.DEMO, motion_threshold=1e6)


def stats(ms):
    ms = np.sort(np.asarray(ms))
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(ms[0]), 4),
            "p90_ms": round(float(ms[int(0.9 * (len(ms) - 1))]), 4), "n": len(ms)}


def gpu(reps):
    import svhip as S
    prm = S.vo_mono_params(f=P["f"], cu=P["cu"], cv=P["cv"], height=P["height"], pitch=P["pitch"],
                           motion_threshold=P["motion_threshold"])
    frames = H.mono_frames()
    out = []
    frame_ms, phases = [], []
    for r in range(reps + 1):
        vo = S.VoMono(prm)
        for k, img in enumerate(frames):
            t0 = time.perf_counter()
            vo.process(img)
            ms = 1e3 * (time.perf_counter() - t0)
            if k and r:   # repetition 0 warms up
                frame_ms.append(ms)
        vo.close()
    out.append(dict(figure="gpu_process_per_frame", frames="I1_000001..6", **stats(frame_ms)))
    for n, seed in ((350, 11), (2000, 12)):
        m = R.synth_scene(n, seed)
        vo = S.VoMono(prm)
        assert vo.process_matches(m)
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            vo.process_matches(m)
            ms.append(1e3 * (time.perf_counter() - t0))
        vo.set_timing(True)
        ph = []
        for _ in range(reps):
            vo.process_matches(m)
            ph.append(vo.timing())
        ph = np.median(np.array(ph), axis=0)
        out.append(dict(figure="gpu_estimate", N=n, inliers=len(vo.inliers()), **stats(ms)))
        out.append(dict(figure="gpu_estimate_device_phases", N=n, ransac_ms=round(float(ph[0]), 4),
                        chirality_ms=round(float(ph[1]), 4), plane_ms=round(float(ph[2]), 4)))
        vo.close()
    return out


def cpu_ref(reps):
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = R.build_harness(tmp)
        R.write_frames(tmp)
        for n, seed in ((350, 11), (2000, 12)):
            m = R.synth_scene(n, seed)
            path = os.path.join(tmp, "m.bin")
            with open(path, "wb") as f:
                f.write(struct.pack("<i", len(m)) + m.tobytes())
            txt = subprocess.run([exe, "bench", tmp, str(reps), path] + R.param_args(R.param_vector(P)),
                                 check=True, capture_output=True, text=True).stdout.split()
            if n == 350:
                out.append(dict(figure="cpu_ref_process_per_frame", median_ms=float(txt[1]), min_ms=float(txt[3]),
                                n=int(txt[5])))
            out.append(dict(figure="cpu_ref_estimate", N=n, median_ms=float(txt[7]), min_ms=float(txt[9])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-ref", action="store_true")
    a = ap.parse_args()
    for line in (cpu_ref(a.reps) if a.cpu_ref else gpu(a.reps)):
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
