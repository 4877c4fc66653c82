"""Writes tests/golden/plane_edges.npz: what the reference's PlaneEstimation (stereomapper/planeestimation.cpp, compiled
unchanged) computes for the cases of plane_ref.edge_cases().  Needs the reference's sources.  Recorded results only, in
the layout of plane.npz: the inputs are closed formulas (plane_ref.list_map, plane_ref.planar_map).

  * list<K>_s3     an empty 640x240 map with d >= 1 on exactly K cells of the lattice, K in 1, 1023, 1024, 1025, 2048:
                   the rounds of 1024 of k_plane_grid and k_plane_select and the tiles of k_plane_vote end there;
  * planar_s3      a noiseless planar road: every sound hypothesis gets every point of the list, so the votes tie at
                   the list length.  Hypothesis 0 is as sound as any other and wins;
  * planar_out_s*  the same road with a quarter of the lattice lifted off the plane: a hypothesis that drew a lifted
                   cell gets fewer votes, the others tie at the number of cells on the road.  The seeds are those for
                   which, in the reference's own votes, the first maximum is not hypothesis 0 and a later hypothesis
                   with as many votes sits in a lower lane of k_plane_select (plane_ref.tie_of).
The reference has 5000 samples built in; every case is recorded with that.

    python tests/golden/make_goldens_plane_edges.py [--search]
"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import plane_ref as R  # noqa: E402

LIMIT = 1024 * 1024


def main():
    out, names = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        exe = R.build_harness(tmp)
        if "--search" in sys.argv:
            for seed in range(0, 12):
                r = R.run_calls(exe, tmp, [(R.planar_map(1024), R.EDGE_W, seed)])[-1]
                print("seed", seed, "best", r["best"], "(h0, h1, votes, ties)", R.tie_of(r["votes"]))
            return
        for name, calls in R.edge_cases():
            r = R.run_calls(exe, tmp, calls)[-1]
            tie = R.tie_of(r["votes"])
            if name.startswith("list"):
                assert len(r["list"]) == int(name[4:name.index("_")]), name
            elif name.startswith("planar_out"):
                assert r["status"] == R.OK and tie and tie[0] == r["best"] > 0 and tie[2] == len(r["list"]) - 1024, (name, tie)
            else:
                assert r["status"] == R.OK and r["best"] == 0 and r["votes"].max() == len(r["list"]) == 4096, name
                assert (r["votes"] == 4096).sum() > 1000, name
            R.pack_result(out, name, r)
            names.append(name)
            print("%-18s status %d n %5d best %5d votes %5d ties %s draws max %4d plane_d %s" % (
                name, r["status"], len(r["list"]), r["best"], r["votes"].max(), tie, r["draws"].max(), r["plane_d"]))
    out["case_names"] = np.array(names)
    out["calib"] = np.array(R.CALIB, np.float32)
    np.savez_compressed(R.EDGE_GOLDEN, **out)
    size = os.path.getsize(R.EDGE_GOLDEN)
    print("wrote %s: %d bytes" % (R.EDGE_GOLDEN, size))
    if size > LIMIT:
        raise SystemExit("plane_edges.npz is larger than %d bytes" % LIMIT)


if __name__ == "__main__":
    main()
