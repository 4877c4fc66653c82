"""Generate the VisualOdometryMono golden fixture (tests/golden/vo_mono.npz).  RUNS ONLY IN THE BUILD CONTAINER.

The reference's own VisualOdometryMono (viso_mono.cpp, compiled unchanged with tests/mono/mono_prelude.h, see
tests/mono_ref.py) is built into a temporary directory and never committed.  Recorded:
  * seq_<name>_*  the seven frames I1_000000..6 through process(I, dims, replace) for the three runs of
                  mono_ref.SEQUENCES: return value, bucketed matches, inlier indices, getDeltaMotion() per frame;
  * est_<name>_*  VisualOdometry::process(p_matched) on a fresh object for the synthetic and degenerate cases of
                  mono_ref.estimate_cases(): matches, return value, inliers, motion, and the inlier count of every
                  RANSAC hypothesis (the loop of estimateMotion replayed on a fresh srand(0) object).

    python tests/golden/make_goldens_mono.py
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import helpers as H  # noqa: E402
import mono_ref as R  # noqa: E402


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = R.build_harness(tmp)
        R.write_frames(tmp)
        out["seq_names"] = np.array([s[0] for s in R.SEQUENCES])
        for name, p, demo_replace in R.SEQUENCES:
            frames = R.run_sequence(exe, tmp, p, demo_replace)
            out["seq_%s_params" % name] = R.param_vector(p)
            out["seq_%s_demo_replace" % name] = np.array(int(demo_replace))
            out["seq_%s_ok" % name] = np.array([f[0] for f in frames], np.int32)
            out["seq_%s_nm" % name] = np.array([len(f[1]) for f in frames], np.int32)
            out["seq_%s_matches" % name] = np.concatenate([f[1] for f in frames])
            out["seq_%s_ni" % name] = np.array([len(f[2]) for f in frames], np.int32)
            out["seq_%s_inliers" % name] = np.concatenate([f[2] for f in frames]).astype(np.int32)
            out["seq_%s_motion" % name] = np.stack([f[3] for f in frames])
            print(name, "ok", out["seq_%s_ok" % name].tolist(), "matches", out["seq_%s_nm" % name].tolist(),
                  "inliers", out["seq_%s_ni" % name].tolist())
        cases = R.estimate_cases()
        out["est_names"] = np.array([c[0] for c in cases])
        for name, pvec, m in cases:
            ok, inl, T, votes = R.run_estimate(exe, tmp, pvec, m)
            out["est_%s_params" % name] = pvec
            out["est_%s_matches" % name] = m
            out["est_%s_ok" % name] = np.array(ok, np.int32)
            out["est_%s_inliers" % name] = inl
            out["est_%s_motion" % name] = T
            out["est_%s_votes" % name] = votes
            print(name, "N", len(m), "ok", ok, "inliers", len(inl), "votes", len(votes),
                  "max", int(votes.max()) if len(votes) else None)
    np.savez_compressed(R.GOLDEN, **out)
    print("vo_mono.npz", os.path.getsize(R.GOLDEN) // 1024, "KiB")


if __name__ == "__main__":
    main()
