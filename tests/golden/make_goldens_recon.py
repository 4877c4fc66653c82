"""Generate the Reconstruction golden fixture (tests/golden/recon.npz).  RUNS ONLY IN THE BUILD CONTAINER.

The reference's own Reconstruction (reconstruction.cpp, compiled unchanged with tests/recon/recon_prelude.h, see
tests/recon_ref.py) is built into a temporary directory and never committed.  Recorded per scene of recon_ref
(frames, synth, edge):
  * <scene>_Tr, _n, _u1p _v1p _i1p _u1c _v1c _i1c   the inputs of every update (so that no test regenerates them);
  * <scene>_settings                                 (point_type, min_track_length, max_dist, min_angle) per run;
  * <scene>_<j>_active, _napp, _points, _nlost, _codes   per update of run j: tracks alive afterwards, the points
    update() appended, and the outcome code of every lost track in the reference's order (the driver derives them
    from the reference's private functions and checks that its ACCEPTED tracks are what update() appended).
Every outcome code 0-6 must occur somewhere, or the script fails.

    python tests/golden/make_goldens_recon.py
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import recon_ref as R  # noqa: E402

LIMIT = 1024 * 1024


def main():
    out = {"calib": np.array(R.CALIB, np.float64), "scene_names": np.array(list(R.SETTINGS))}
    seen = np.zeros(7, np.int64)
    with tempfile.TemporaryDirectory() as tmp:
        exe = R.build_harness(tmp)
        scenes = {"frames": R.frames_scene(tmp), "synth": R.synth_scene(), "edge": R.edge_scene()}
        for name, scene in scenes.items():
            R.pack_scene(out, name, scene)
            out[name + "_settings"] = np.array(R.SETTINGS[name], np.float64)
            path = os.path.join(tmp, name + ".bin")
            R.write_scene(path, scene)
            for j, s in enumerate(R.SETTINGS[name]):
                res = R.run_scene(exe, path, len(scene), s)
                R.pack_result(out, "%s_%d" % (name, j), res)
                codes = np.concatenate([r[2] for r in res])
                hist = np.bincount(codes, minlength=7)
                seen += hist
                print(name, s, "updates", len(scene), "matches", sum(len(m) for _, m in scene), "lost", len(codes),
                      "longest", max(len(m) for _, m in scene), dict(zip(R.CODE_NAMES, hist.tolist())))
                print("   reference:", R.run_bench(exe, path, s, 5))
    missing = [R.CODE_NAMES[c] for c in range(7) if seen[c] == 0]
    if missing:
        raise SystemExit("outcome codes that never occur: %s" % missing)
    np.savez_compressed(R.GOLDEN, **out)
    size = os.path.getsize(R.GOLDEN)
    print("recon.npz", size // 1024, "KiB")
    if size > LIMIT:
        raise SystemExit("recon.npz is larger than %d bytes: lower recon_ref.SYNTH_POINTS" % LIMIT)


if __name__ == "__main__":
    main()
