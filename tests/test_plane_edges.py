"""CPU: the cases of tests/golden/plane_edges.npz (make_goldens_plane_edges.py, plane_ref.edge_cases): lattice lists of
exactly 1, 1023, 1024, 1025 and 2048 entries -- where the rounds of k_plane_grid and k_plane_select and the tiles of
k_plane_vote end -- and noiseless planar roads on which the votes of many hypotheses tie.

Asserted on the recorded votes and on the maps as plane_ref builds them: the exact list lengths; on the planar road a
tie of more than 1000 hypotheses at the full list length (hypothesis 0 is as sound as any other there and wins); on
the road with a quarter of its cells lifted off the plane a winner that is NOT hypothesis 0 and a later hypothesis
with as many votes in a lower lane of k_plane_select (h1 % 1024 < h0 % 1024), the arrangement in which a reduction
that prefers the lower lane to the lower index returns another hypothesis.  best is compared by the GPU tests, so the
wrong choice shows whatever its inliers are.

Then the live reference and plane_core.h against the record, as tests/test_plane.py does for plane.npz.  The GPU runs
are in tests/test_plane_edges_gpu.py."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import plane_ref as R
from test_plane import CORE_CHECK, core_run


@pytest.fixture(scope="module")
def Z():
    with np.load(R.EDGE_GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_fixture_has_the_lengths_and_the_ties(Z):
    assert os.path.getsize(R.EDGE_GOLDEN) <= 1024 * 1024
    cases = R.edge_cases()
    assert list(Z["case_names"]) == [n for n, _ in cases]
    assert tuple(Z["calib"]) == tuple(np.float32(c) for c in R.CALIB)
    assert R.EDGE_LENGTHS == (1, 1023, 1024, 1025, 2048)
    by_name = dict(cases)
    for k in R.EDGE_LENGTHS:
        name = "list%d_s%d" % (k, R.EDGE_SEED)
        D = by_name[name][0][0]
        r = R.unpack_result(Z, name)
        assert r["n"] == k == int((D >= 1).sum()), name                         # every kept pixel is a lattice cell
        cu, cv = R.edge_cells(k)
        assert len(cu) == k and (D[cv, cu] >= 1).all() and (cu % 5 == 0).all() and ((cv - R.EDGE_H // 3) % 5 == 0).all()
        assert len(r["votes"]) == R.NUM_SAMPLES
        if k > 1:
            assert r["status"] == R.OK and 3 < r["votes"].max() < k and r["best"] == int(np.argmax(r["votes"])) > 0
    one = R.unpack_result(Z, "list1_s%d" % R.EDGE_SEED)
    assert one["status"] == R.FEW_INLIERS and (one["draws"] == 1000).all()
    flat = R.unpack_result(Z, "planar_s%d" % R.EDGE_SEED)
    assert flat["n"] == R.EDGE_NU * R.EDGE_NV == 4096 and flat["best"] == 0
    assert flat["votes"].max() == flat["n"] and (flat["votes"] == flat["n"]).sum() > 1000
    assert len(R.EDGE_TIE_SEEDS) >= 2
    for seed in R.EDGE_TIE_SEEDS:
        r = R.unpack_result(Z, "planar_out_s%d" % seed)
        tie = R.tie_of(r["votes"])
        assert tie is not None, seed
        h0, h1, most, reach = tie
        assert h0 == r["best"] == int(np.argmax(r["votes"])) and h0 > 0                 # the winner is not hypothesis 0
        assert h1 > h0 and h1 % 1024 < h0 % 1024 and r["votes"][h1] == most
        assert most == r["n"] - 1024 == len(r["inliers"]) and reach > 1000              # every cell on the road, many times


def test_plane_core_reproduces_edges(Z, tmp_path):
    exe = str(tmp_path / "plane_core_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe, CORE_CHECK])
    for name, calls in R.edge_cases():
        got = core_run(exe, tmp_path, calls)[-1]
        R.same_result(got, R.unpack_result(Z, name), name)


@pytest.mark.skipif(not R.have_ref(), reason="the reference's sources are not on this machine")
def test_live_reference_equals_edges(Z):
    with tempfile.TemporaryDirectory() as tmp:
        exe = R.build_harness(tmp)
        for name, calls in R.edge_cases():
            got = R.run_calls(exe, tmp, calls)[-1]
            R.same_result(got, R.unpack_result(Z, name), name)
