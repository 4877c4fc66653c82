"""Generate tests/golden/recon_collide.npz: one more Reconstruction scene, `collide`, in the layout of recon.npz
(make_goldens_recon.py).  RUNS ONLY IN THE BUILD CONTAINER.

recon.npz and recon_shared.npz come from realistic drives: their sizes and collisions are whatever those drives
produced.  This scene (recon_ref.collide_scene) has the ones at which the kernels of the resident track table
(recon_track_kernels.hip) can go wrong:
  * n and n_old walk through 1023, 1024, 1025, 2048, 2049 and 3000 (k_rt_scan gives each of 1024 threads a run of
    ceil(n/1024)), then 0 -- every one of 3000 tracks is lost, twelve rounds of k_rt_compact -- then 1; the update
    before the empty one extends every one of its 2049 old tracks;
  * feature indices on which two or three tracks end whose numbers lie in different blocks of 256 (k_rt_scatter's
    atomicMax across workgroups), each asked for by a match of the next update;
  * i1p values named by two to four matches in different blocks of 256 (k_rt_associate's atomicMin across
    workgroups), a third of them on the shared indices above;
  * feature indices below 60000 in some frames and below the number of features in others.
The script asserts all of that on its own serial replay (recon_ref.sequential_update) before it records the
reference's results; tests/test_recon_collide.py asserts it again on the stored inputs with the parallel form.

The reference's own Reconstruction is built through recon_ref.build_harness into a temporary directory and never
committed.

    python tests/golden/make_goldens_recon_collide.py
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import recon_ref as R  # noqa: E402

LIMIT = 1024 * 1024
OUT = R.COLLIDE_GOLDEN


def main():
    scene = R.collide_scene()
    p = R.collide_properties(scene, R.sequential_update)
    print({k: (v if not isinstance(v, list) or len(v) < 20 else len(v)) for k, v in p.items()})
    R.check_collide_properties(p)
    out = {"calib": np.array(R.CALIB, np.float64), "scene_names": np.array(["collide"])}
    with tempfile.TemporaryDirectory() as tmp:
        exe = R.build_harness(tmp)
        R.pack_scene(out, "collide", scene)
        out["collide_settings"] = np.array(R.COLLIDE_SETTINGS, np.float64)
        path = os.path.join(tmp, "collide.bin")
        R.write_scene(path, scene)
        for j, s in enumerate(R.COLLIDE_SETTINGS):
            res = R.run_scene(exe, path, len(scene), s)
            R.pack_result(out, "collide_%d" % j, res)
            codes = np.concatenate([r[2] for r in res])
            print(s, "lost", [len(r[2]) for r in res], dict(zip(R.CODE_NAMES, np.bincount(codes, minlength=7).tolist())))
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print("recon_collide.npz", size // 1024, "KiB")
    if size > LIMIT:
        raise SystemExit("recon_collide.npz is larger than %d bytes" % LIMIT)


if __name__ == "__main__":
    main()
