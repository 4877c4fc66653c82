"""Timing of VisualOdometryMono (svh_vo_mono_*): ms per process() over the reference's seven mono frames, ms per
estimate-only call (VisualOdometry::process(p_matched)) at N = 350 and N = 2000, and the device time of the
estimate's three phases from HIP events (RANSAC: k_mono_hyp + k_mono_vote + k_mono_select; chirality:
k_mono_chiral + k_mono_pick; plane vote: k_mono_plane; each with its upload).  One JSON line per figure.

    python tools/gpu_mono_vo.py [--reps R]            on the GPU
    python tools/gpu_mono_vo.py --cpu-ref [--reps R]  the reference on the CPU, measured the same way (needs the
                                                      reference's sources: build machine only)
    python tools/gpu_mono_vo.py --lockstep 1,4,16,32  K objects through svh_vo_mono_process_batch against the same K
                                                      objects through a loop of svh_vo_mono_process (below)

Method: a host clock around calls that end in a device synchronise.  process(): a fresh object per repetition
(outside the clock), frames 0-6 in order, frames 1-6 timed (frame 0 only fills the ring buffer), the calibration
of demo_viso_mono.m with motion_threshold 1e6 so that every estimate runs to the end.  Estimate-only: the seeded
synthetic scenes of tests/mono_ref.py (20 % outliers), one object, R calls after one untimed call.

--lockstep: two sets of K objects with private random streams (seed 0), one driven through the lockstep entry, one
through the loop of single calls, ALTERNATING frame by frame in one process; the same frames and parameters as above.
Per repetition the seven frames in order, frames 1-6 timed; the objects live across repetitions (repetition 0 warms
up).  Figures per K: ms per call of either form (one call = one frame of K sequences) and frames/s = K / median; the
device time of the three phases of the whole batch (HIP events, a pass of its own with timing on); the same for the
estimate alone (svh_vo_mono_process_matches_batch against a loop of svh_vo_process_matches) at N = 350 and N = 2000.
Every line is also appended to --out (profiles/mono_lockstep_times.jsonl)."""
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


def lockstep(ks, reps):
    import svhip as S
    prm = S.vo_mono_params(f=P["f"], cu=P["cu"], cv=P["cv"], height=P["height"], pitch=P["pitch"],
                           motion_threshold=P["motion_threshold"])
    frames = [np.ascontiguousarray(f, np.uint8) for f in H.mono_frames()]
    rate = lambda K, st: round(1e3 * K / st["median_ms"], 1)
    for K in ks:
        bat = [S.VoMono(prm, private_rand=0) for _ in range(K)]
        loop = [S.VoMono(prm, private_rand=0) for _ in range(K)]
        t_b, t_l, good = [], [], 0
        for r in range(reps + 1):
            for k, img in enumerate(frames):
                t0 = time.perf_counter()
                ok = S.VoMono.process_batch(bat, [img] * K)
                t1 = time.perf_counter()
                for vo in loop:
                    vo.process(img)
                t2 = time.perf_counter()
                if k and r:
                    t_b.append(1e3 * (t1 - t0))
                    t_l.append(1e3 * (t2 - t1))
                    good += sum(ok)
        sb, sl = stats(t_b), stats(t_l)
        yield dict(figure="lockstep_process_per_call", K=K, form="svh_vo_mono_process_batch", frames_per_s=rate(K, sb),
                   motions_updated=good, **sb)
        yield dict(figure="lockstep_process_per_call", K=K, form="loop of svh_vo_mono_process",
                   frames_per_s=rate(K, sl), **sl)
        for vo in bat:
            vo.set_timing(True)
        ph = []
        for r in range(max(reps // 4, 3)):
            for k, img in enumerate(frames):
                S.VoMono.process_batch(bat, [img] * K)
                if k:
                    ph.append(bat[0].timing())
        ph = np.median(np.array(ph), axis=0)
        yield dict(figure="lockstep_process_device_phases", K=K, ransac_ms=round(float(ph[0]), 4),
                   chirality_ms=round(float(ph[1]), 4), plane_ms=round(float(ph[2]), 4))
        for vo in bat + loop:
            vo.set_timing(False)
        for n, seed in ((350, 11), (2000, 12)):
            m = R.synth_scene(n, seed)
            ms = [m] * K
            assert all(S.VoMono.process_matches_batch(bat, ms)) and all(vo.process_matches(m) for vo in loop)
            t_b, t_l = [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                S.VoMono.process_matches_batch(bat, ms)
                t1 = time.perf_counter()
                for vo in loop:
                    vo.process_matches(m)
                t2 = time.perf_counter()
                t_b.append(1e3 * (t1 - t0))
                t_l.append(1e3 * (t2 - t1))
            sb, sl = stats(t_b), stats(t_l)
            for vo in bat:
                vo.set_timing(True)
            ph = []
            for _ in range(max(reps // 2, 3)):
                S.VoMono.process_matches_batch(bat, ms)
                ph.append(bat[0].timing())
            for vo in bat:
                vo.set_timing(False)
            ph = np.median(np.array(ph), axis=0)
            yield dict(figure="lockstep_estimate_per_call", K=K, N=n, form="svh_vo_mono_process_matches_batch",
                       estimates_per_s=rate(K, sb), **sb)
            yield dict(figure="lockstep_estimate_per_call", K=K, N=n, form="loop of svh_vo_process_matches",
                       estimates_per_s=rate(K, sl), **sl)
            # what of a batch call is not device time of the three phases: the per-object host steps (samples, refit,
            # nth_element), the recording and the waits' latency
            yield dict(figure="lockstep_estimate_device_phases", K=K, N=n, ransac_ms=round(float(ph[0]), 4),
                       chirality_ms=round(float(ph[1]), 4), plane_ms=round(float(ph[2]), 4),
                       host_and_latency_ms=round(sb["median_ms"] - float(ph.sum()), 4))
        for vo in bat + loop:
            vo.close()


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
    ap.add_argument("--lockstep", default=None, help="K[,K...]: the lockstep entries against the loop of single calls")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mono_lockstep_times.jsonl"))
    a = ap.parse_args()
    if a.lockstep:
        with open(a.out, "a") as f:
            for line in lockstep([int(k) for k in a.lockstep.split(",")], max(a.reps, 20)):
                print(json.dumps(line), flush=True)
                f.write(json.dumps(line) + "\n")
                f.flush()
        return
    for line in (cpu_ref(a.reps) if a.cpu_ref else gpu(a.reps)):
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
