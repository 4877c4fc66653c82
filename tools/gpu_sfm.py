"""Timing of the structure-from-motion loop (libviso2/matlab/demo_structure_from_motion.m:29-67: mono visual odometry
on a frame, then Reconstruction::update on the same frame) for K sequences at once, and of Reconstruction's update
alone in its four forms.  One JSON line per figure, each also appended to a file under profiles/.

    python tools/gpu_sfm.py --lockstep 1,4,16 [--reps R]
        K VisualOdometryMono objects through svh_vo_mono_process_batch, then K resident Reconstruction objects through
        svh_recon_update_batch with update(matches, Tr, 2, 2, 30, 3); a sequence whose odometry failed sits the
        reconstruction out (NULL matches) and gets replace = 1 on its next frame.  Against it, in the same process and
        alternating frame by frame, K objects through a loop of svh_vo_mono_process + svh_recon_update (host table).
        The reference's seven mono frames, frames 1-6 timed, repetition 0 warms up.  -> profiles/sfm_lockstep_times.jsonl

    python tools/gpu_sfm.py --recon FORM --scene SCENE [--pkg DIR] [--reps R]
        ms per update of Reconstruction alone.  FORM: batch (K = 16 resident objects, svh_recon_update_batch),
        loop_host (16 svh_recon_update calls on host-table objects), resident (one resident object), host (one
        host-table object).  SCENE: synth4000 (recon_ref.synth_scene scaled to about 4 000 matches per update), synth,
        frames, edge (tests/golden/recon.npz).  --pkg DIR imports svhip from DIR (a build of another commit: loop_host
        and host use only entries every build has).  Fresh objects per repetition, every update timed (all K objects
        get the scene's update k in one timed step), repetition 0 thrown away.  -> profiles/recon_resident_times.jsonl

Method: a host clock around calls that end in a stream wait."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

K_RECON = 16
SETTING = (1, 2, 30.0, 2.0)     # update()'s defaults, what tools/gpu_recon.py times
DEMO_SETTING = (2, 2, 30.0, 3.0)   # demo_structure_from_motion.m:63


def stats(ms):
    ms = np.sort(np.asarray(ms))
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(ms[0]), 4),
            "p90_ms": round(float(ms[int(0.9 * (len(ms) - 1))]), 4), "n": len(ms)}


def emit(path, line):
    print(json.dumps(line), flush=True)
    with open(path, "a") as f:
        f.write(json.dumps(line) + "\n")


def recon_scene(name):
    import recon_ref as R
    if name == "synth4000":
        # 20 000 points over 16 updates: 1 200 matches in the first update, 3 700 - 4 100 from the eighth on
        return [(Tr, R.to_p_match(m)) for Tr, m in R.synth_scene(n_points=20000, n_updates=16)], R.CALIB
    with np.load(R.GOLDEN) as z:
        Z = {k: z[k] for k in z.files}
    return [(Tr, R.to_p_match(m)) for Tr, m in R.unpack_scene(Z, name)], tuple(float(c) for c in Z["calib"])


def recon_times(form, scene_name, pkg, reps, out):
    sys.path.insert(0, pkg)
    import svhip as S
    scene, calib = recon_scene(scene_name)
    K = K_RECON if form in ("batch", "loop_host") else 1
    resident = form in ("batch", "resident")
    ms, points = [], 0
    for r in range(reps + 1):
        objs = [S.Reconstruction(resident=True) if resident else S.Reconstruction() for _ in range(K)]
        for o in objs:
            o.set_calibration(*calib)
        for Tr, m in scene:
            t0 = time.perf_counter()
            if form == "batch":
                S.Reconstruction.update_batch(objs, [m] * K, [Tr] * K, *SETTING)
            else:
                for o in objs:
                    o.update(m, Tr, *SETTING)
            if r:
                ms.append(1e3 * (time.perf_counter() - t0))
        points = objs[-1].num_points()
        for o in objs:
            o.close()
    emit(out, dict(figure="recon_update", form=form, K=K, scene=scene_name, build=S.lib().svh_version().decode(),
                   updates=len(scene), matches_per_update_median=int(np.median([len(m) for _, m in scene])),
                   points=points, per_object_ms=round(float(np.median(ms)) / K, 4), **stats(ms)))


def lockstep(ks, reps, out):
    sys.path.insert(0, os.path.join(ROOT, "stereo-vision_amd"))
    import helpers as H
    import mono_ref
    import svhip as S
    P = dict(mono_ref.DEMO, motion_threshold=1e6)
    prm = S.vo_mono_params(f=P["f"], cu=P["cu"], cv=P["cv"], height=P["height"], pitch=P["pitch"],
                           motion_threshold=P["motion_threshold"])
    frames = [np.ascontiguousarray(f, np.uint8) for f in H.mono_frames()]
    calib = (P["f"], P["cu"], P["cv"])
    for K in ks:
        t_b, t_l, updates, pts = [], [], 0, (0, 0)
        for r in range(reps + 1):
            vb = [S.VoMono(prm, private_rand=0) for _ in range(K)]
            vl = [S.VoMono(prm, private_rand=0) for _ in range(K)]
            rb = [S.Reconstruction(resident=True) for _ in range(K)]
            rl = [S.Reconstruction() for _ in range(K)]
            for o in rb + rl:
                o.set_calibration(*calib)
            rep_b, rep_l = [0] * K, [0] * K
            for k, img in enumerate(frames):
                t0 = time.perf_counter()
                ok = S.VoMono.process_batch(vb, [img] * K, replace=rep_b)
                if k:
                    S.Reconstruction.update_batch(rb, [v.matches() if g else None for v, g in zip(vb, ok)],
                                                  [v.motion() if g else None for v, g in zip(vb, ok)], *DEMO_SETTING)
                    rep_b = [0 if g else 1 for g in ok]
                t1 = time.perf_counter()
                for i, (v, o) in enumerate(zip(vl, rl)):
                    g = v.process(img, replace=rep_l[i])
                    if k:
                        if g:
                            o.update(v.matches(), v.motion(), *DEMO_SETTING)
                        rep_l[i] = 0 if g else 1
                t2 = time.perf_counter()
                if k and r:
                    t_b.append(1e3 * (t1 - t0))
                    t_l.append(1e3 * (t2 - t1))
                    updates += sum(ok)
            pts = (rb[0].num_points(), rl[0].num_points())
            for o in vb + vl + rb + rl:
                o.close()
        sb, sl = stats(t_b), stats(t_l)
        emit(out, dict(figure="sfm_per_frame", K=K, form="svh_vo_mono_process_batch + svh_recon_update_batch",
                       frames_per_s=round(1e3 * K / sb["median_ms"], 1), updates=updates, points=pts[0], **sb))
        emit(out, dict(figure="sfm_per_frame", K=K, form="loop of svh_vo_mono_process + svh_recon_update",
                       frames_per_s=round(1e3 * K / sl["median_ms"], 1), points=pts[1], **sl))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--lockstep", default=None, help="K[,K...]: the demo loop for K sequences")
    ap.add_argument("--recon", default=None, choices=["batch", "loop_host", "resident", "host"])
    ap.add_argument("--scene", default="synth4000", choices=["synth4000", "synth", "frames", "edge"])
    ap.add_argument("--pkg", default=os.path.join(ROOT, "stereo-vision_amd"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.recon:
        recon_times(a.recon, a.scene, a.pkg, a.reps, a.out or os.path.join(ROOT, "profiles", "recon_resident_times.jsonl"))
    elif a.lockstep:
        lockstep([int(k) for k in a.lockstep.split(",")], a.reps,
                 a.out or os.path.join(ROOT, "profiles", "sfm_lockstep_times.jsonl"))
    else:
        ap.error("--lockstep or --recon")


if __name__ == "__main__":
    main()
