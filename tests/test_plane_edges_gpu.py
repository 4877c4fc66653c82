"""GPU: the cases of tests/golden/plane_edges.npz (what they contain is asserted in tests/test_plane_edges.py) through
k_plane_grid, k_plane_fit, k_plane_vote and k_plane_select, against the reference's record: from a host map, from a
device map, and in one svh_plane_estimate_batch beside an urban map.  Only committed fixtures are read; the maps are
plane_ref's closed formulas.

Compared with plane_ref.same_result, as tests/test_plane_gpu.py does: status, list, draws, every vote, the winner,
its inliers, and every double as a bit pattern.  No tolerance.

The reference has 5000 samples built in.  Sample counts 1, 255, 257 and 1025 -- off the 256 hypotheses of a
k_plane_vote workgroup and the 1024 lanes of k_plane_select -- are compared with plane_core.h on the host
(tests/plane/plane_core_check.cpp compiled on the spot), on a map whose votes tie and on a list of 1025 entries."""
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import plane_ref as R
from test_plane_gpu import DevMap, got_of, run_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Z():
    out = R.load_golden()
    with np.load(R.EDGE_GOLDEN) as z:
        out.update({k: z[k] for k in z.files if k not in ("case_names", "calib")})
    return out


@pytest.fixture(scope="module")
def S():
    import svhip
    return svhip


@pytest.fixture(scope="module")
def hip():
    import ctypes as C
    return C.CDLL("libamdhip64.so")


def test_every_case_from_host_and_device_maps(S, Z, hip):
    for name, calls in R.edge_cases():
        want = R.unpack_result(Z, name)
        for where in (None, hip):
            pl = S.PlaneEstimation()
            rc = run_case(pl, calls, where)
            R.same_result(got_of(pl, rc), want, (name, "host" if where is None else "device"))
            pl.close()


def test_batch_beside_an_urban_map(S, Z, hip):
    """maps of one size run in one batch: the 640x240 cases together (lists of 1 to 4096 entries side by side), and
    each embedded in the bottom left corner of an empty 1242x375 frame beside urban2: the lists keep their lengths
    (the cells stay on the lattice) with other coordinates, so those are compared with a single call."""
    cases = R.edge_cases()
    maps = [DevMap(hip, calls[0][0]) for _, calls in cases]
    objs = [S.PlaneEstimation() for _ in cases]
    try:
        st = S.PlaneEstimation.estimate_batch(objs, [m.addr for m in maps], R.EDGE_W, R.EDGE_H, R.EDGE_W,
                                              seeds=[calls[0][2] for _, calls in cases])
        for (name, _), o, rc in zip(cases, objs, st):
            R.same_result(got_of(o, rc), R.unpack_result(Z, name), ("batch", name))
    finally:
        for m in maps:
            m.free()
        for o in objs:
            o.close()
    # beside an urban map: the urban map against the reference's record, the embedded ones against single calls
    urban = R.urban_d1("urban2_stereomapper")
    big = []
    for _, calls in cases:
        D = np.zeros((R.HGT, R.W), np.float32)
        D[R.HGT - R.EDGE_H:, :R.EDGE_W] = calls[0][0]
        big.append((D, calls[0][2]))
    jobs = big[:4] + [(urban, 2)] + big[4:]
    maps = [DevMap(hip, D) for D, _ in jobs]
    objs = [S.PlaneEstimation() for _ in jobs]
    try:
        st = S.PlaneEstimation.estimate_batch(objs, [m.addr for m in maps], R.W, R.HGT, R.W, seeds=[s for _, s in jobs])
        R.same_result(got_of(objs[4], st[4]), R.unpack_result(Z, "urban2_stereomapper_s2"), "urban beside the edges")
        lengths = set()
        for k, ((D, seed), o, rc) in enumerate(zip(jobs, objs, st)):
            if k == 4:
                continue
            one = S.PlaneEstimation()
            want = got_of(one, one.estimate(D, width=R.W, seed=seed))
            got = got_of(o, rc)
            assert got["status"] == want["status"] and got["best"] == want["best"], k
            for key in ("list", "draws", "votes", "inliers"):
                assert np.array_equal(got[key], want[key]), (k, key)
            for key in ("planes", "plane_d", "plane_e", "H"):
                assert np.ascontiguousarray(got[key], np.float64).tobytes() == \
                    np.ascontiguousarray(want[key], np.float64).tobytes(), (k, key)
            lengths.add(len(got["list"]))
            one.close()
        assert {1, 1023, 1024, 1025, 2048} <= lengths, sorted(lengths)
    finally:
        for m in maps:
            m.free()
        for o in objs:
            o.close()


@pytest.mark.parametrize("samples", [1, 255, 257, 1025])
def test_sample_counts_off_the_block_sizes_match_the_host_core(S, tmp_path, samples):
    exe = str(tmp_path / "plane_core_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe,
                           os.path.join(H.ROOT, "tests", "plane", "plane_core_check.cpp")])
    for what, D, seed in (("tied", R.planar_map(1024), R.EDGE_TIE_SEEDS[0]), ("list1025", R.list_map(1025), R.EDGE_SEED)):
        path = str(tmp_path / "job.bin")
        R.write_job(path, [(D, R.EDGE_W, seed)])
        want = R.parse_run(subprocess.run([exe, path, str(samples), "5", "50", "1000"], check=True,
                                          capture_output=True).stdout, 1)[0]
        assert len(want["votes"]) == samples and len(want["list"]) in (4096, 1025)
        pl = S.PlaneEstimation(num_samples=samples)
        rc = pl.estimate(D, width=R.EDGE_W, seed=seed)
        got = got_of(pl, rc)
        assert rc == want["status"], (what, samples)
        for k in ("list", "draws", "votes", "inliers"):
            assert np.array_equal(got[k], want[k]), (what, samples, k)
        assert got["best"] == want["best"], (what, samples)
        for k in ("planes", "plane_d", "plane_e", "H"):
            assert np.ascontiguousarray(got[k], np.float64).tobytes() == want[k].tobytes(), (what, samples, k)
        assert np.float32(got["pitch"]).tobytes() == np.float32(want["pitch"]).tobytes()
        pl.close()
