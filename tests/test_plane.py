"""CPU: PlaneEstimation's golden fixture (tests/golden/plane.npz, make_goldens_plane.py), the numeric core of the
kernels and the engine (stereo-vision_amd/csrc/plane_core.h) against it, a live run of the reference when its sources
are present, the drop-in header include/planeestimation.h, the glibc rand() anchor and the misuse cases of the C-ABI
that need no device.

plane_core.h performs the reference's operations in the reference's order and formats and is built here by the same
compiler family without FMA contraction, so equality is the derived expectation: list, draws, votes, winner and inlier
indices identical, every double bit-equal, no tolerance."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import helpers as H
import plane_ref as R

CORE_CHECK = os.path.join(H.ROOT, "tests", "plane", "plane_core_check.cpp")


@pytest.fixture(scope="module")
def Z():
    return R.load_golden()


def test_fixture_covers_the_cases_and_stays_small(Z):
    assert os.path.getsize(R.GOLDEN) <= 662315                   # the largest fixture before this one (recon.npz)
    names = [n for n, _ in R.cases()]
    assert list(Z["case_names"]) == names and len(names) == 21
    assert tuple(Z["calib"]) == tuple(np.float32(c) for c in R.CALIB)
    for name in names:
        r = R.unpack_result(Z, name)
        assert len(r["draws"]) == len(r["votes"]) == R.NUM_SAMPLES
        assert (r["best"] >= 0) == (len(r["inliers"]) > 0)
        if r["best"] >= 0:
            assert r["votes"][r["best"]] == len(r["inliers"]) == r["votes"].max()
            assert r["best"] == int(np.argmax(r["votes"]))       # the first maximum
        assert (r["status"] == R.OK) == (len(r["inliers"]) > 3)
    # the branches the cases are there for (make_goldens_plane.py asserts them on the reference's output)
    eye = np.eye(4)
    for name in names:
        r = R.unpack_result(Z, name)
        if name.startswith(("urban", "embedded", "half")):
            assert abs(r["plane_d"][1]) > 0.1 and not np.array_equal(r["H"], eye)
        if name.startswith("wall"):
            assert abs(r["plane_d"][1]) <= 0.1 and np.array_equal(r["H"], eye)
            assert r["pitch"] == R.unpack_result(Z, "urban2_stereomapper_s2")["pitch"] != 0
        if name.startswith("small"):
            assert (r["draws"] == 1000).any()
        if name.startswith(("two", "three")):
            assert r["status"] == R.FEW_INLIERS and np.array_equal(r["H"], eye) and not r["plane_e"].any()
    assert np.array_equal(Z["embedded_s2_plane_d"], Z["urban2_stereomapper_s2_plane_d"])


def test_seed_0_and_seed_1_are_the_same_stream():
    """glibc's srand(0) seeds as srand(1); the library's private generator says the same, and its first draws of
    srand(1) are glibc's well-known ones"""
    import svhip as S
    L = S.lib()
    L.svh_rand_sequence.argtypes = [C.c_uint32, C.c_void_p, C.c_int32]
    L.svh_rand_sequence.restype = None
    a, b, c = (np.zeros(4096, np.int32) for _ in range(3))
    L.svh_rand_sequence(0, a.ctypes.data, len(a))
    L.svh_rand_sequence(1, b.ctypes.data, len(b))
    L.svh_rand_sequence(2, c.ctypes.data, len(c))
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert list(b[:5]) == [1804289383, 846930886, 1681692777, 1714636915, 1957747793]


def core_run(exe, tmp, calls, extra=()):
    path = os.path.join(str(tmp), "job.bin")
    R.write_job(path, calls)
    b = subprocess.run([exe, path] + [str(x) for x in extra], check=True, capture_output=True).stdout
    return R.parse_run(b, len(calls))


def test_plane_core_reproduces_reference(Z, tmp_path):
    """plane_core.h built by g++ -ffp-contract=off: every case of the fixture, everything identical"""
    exe = str(tmp_path / "plane_core_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe, CORE_CHECK])
    for name, calls in R.cases():
        got = core_run(exe, tmp_path, calls)[-1]
        R.same_result(got, R.unpack_result(Z, name), name)


@pytest.mark.skipif(not R.have_ref(), reason="the reference's sources are not on this machine")
def test_live_reference_equals_goldens(Z):
    with tempfile.TemporaryDirectory() as tmp:
        exe = R.build_harness(tmp)
        for name, calls in R.cases():
            got = R.run_calls(exe, tmp, calls)[-1]
            R.same_result(got, R.unpack_result(Z, name), name)


def test_dropin_compiles_against_include_alone(tmp_path):
    """stereothread.cpp:155-163 written against stereomapper/planeestimation.h compiles with include/ only"""
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-I" + os.path.join(H.ROOT, "include"), "-c",
                           os.path.join(H.ROOT, "tests", "plane", "plane_dropin.cpp"), "-o", str(tmp_path / "d.o")])


def test_misuse_is_refused_without_a_device():
    import svhip as S
    P = S.PlaneParams()
    L = S.lib()
    L.svh_plane_params_default(C.byref(P))
    assert (P.num_samples, P.step_size, P.max_draws, list(P.roi), P.min_dist, P.d_threshold) == \
        (5000, 5, 1000, [-1, -1, -1, -1], 50.0, 5.0)
    P.num_samples = 0
    L.svh_plane_create.restype = C.c_void_p
    L.svh_plane_create.argtypes = [C.c_void_p]
    assert not L.svh_plane_create(C.byref(P))
    pl = S.PlaneEstimation()
    D = np.ones((10, 10), np.float32)
    with pytest.raises(S.SvhError) as e:
        pl.estimate(D, width=20)                       # step < width
    assert e.value.code == S.ERR_BAD_ARG
    assert not pl.plane_dsi().any() and np.array_equal(pl.transformation(), np.eye(4)) and pl.pitch() == 0
    pl.close()
