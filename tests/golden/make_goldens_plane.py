"""Writes tests/golden/plane.npz: what the reference's PlaneEstimation (stereomapper/planeestimation.cpp, compiled
unchanged) computes for the cases of tests/plane_ref.py.  Needs the reference's sources (REF, default
/root/reference).  Recorded results only: the inputs are committed `d1` maps or closed formulas (plane_ref.cases).

    python tests/golden/make_goldens_plane.py [--check]     (--check: compare with the committed file, write nothing)

Every case must take the branch it is there for IN THE REFERENCE'S OWN OUTPUT; the assertions below stop the script
otherwise, so that no case passes by missing its subject."""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import plane_ref as R  # noqa: E402

IDENTITY = np.eye(4)


def check_branch(name, res):
    r = res[-1]
    zero_planes = (r["planes"] == 0).all(axis=1)
    if name.startswith("urban") or name.startswith("embedded") or name.startswith("half"):
        assert r["status"] == R.OK and abs(r["plane_d"][1]) > 0.1 and not np.array_equal(r["H"], IDENTITY), name
        assert abs(float(r["pitch"])) > 1e-3, name
    elif name.startswith("wall"):
        road = res[0]
        assert road["status"] == R.OK and abs(road["plane_d"][1]) > 0.1, name
        assert r["status"] == R.OK and abs(r["plane_d"][1]) <= 0.1 and np.array_equal(r["H"], IDENTITY), (name, r["plane_d"])
        assert r["pitch"] == road["pitch"] and float(r["pitch"]) != 0.0, name
        assert (r["plane_e"] != 0).any(), name
    elif name.startswith("small"):
        assert (r["draws"] == 1000).sum() > 0 and zero_planes.sum() > 0, name      # failed solves -> zero plane
    elif name.startswith("lowd"):
        full = zero_planes & (r["votes"] == len(r["list"]))
        assert full.any() and (r["list"][:, 2] < 5).all() and (r["list"][:, 2] >= 1).all(), name
        assert r["votes"].max() == len(r["list"]), name
    elif name.startswith("two") or name.startswith("three"):
        want_n = 2 if name.startswith("two") else 3
        assert len(r["list"]) == want_n and r["status"] == R.FEW_INLIERS and len(r["inliers"]) <= 3, name
        assert np.array_equal(r["H"], IDENTITY) and (r["plane_e"] == 0).all(), name
        assert np.array_equal(r["plane_d"], r["planes"][-1]), name                 # the LAST hypothesis' plane
    else:
        raise AssertionError("no branch check for " + name)


def main():
    check_only = "--check" in sys.argv
    out = {}
    names = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = R.build_harness(tmp)
        for name, calls in R.cases():
            res = R.run_calls(exe, tmp, calls)
            check_branch(name, res)
            R.pack_result(out, name, res[-1])
            names.append(name)
            r = res[-1]
            print("%-26s status %d n %5d best %5d votes %5d draws max %4d plane_d %s pitch %.10f" % (
                name, r["status"], len(r["list"]), r["best"], r["votes"].max(), r["draws"].max(), r["plane_d"], r["pitch"]))
    out["case_names"] = np.array(names)
    out["calib"] = np.array(R.CALIB, np.float32)
    if check_only:
        Z = R.load_golden()
        assert sorted(Z) == sorted(out), "the fixture has other arrays"
        for k in out:
            assert np.asarray(out[k]).tobytes() == Z[k].tobytes() and np.asarray(out[k]).dtype == Z[k].dtype, k
        print("plane.npz: every array is content-equal to what the reference gives today")
        return
    np.savez_compressed(R.GOLDEN, **out)
    print("wrote %s: %d bytes" % (R.GOLDEN, os.path.getsize(R.GOLDEN)))


if __name__ == "__main__":
    main()
