"""CPU: Reconstruction's golden fixture (tests/golden/recon.npz, make_goldens_recon.py), the numeric core of the
device kernel (stereo-vision_amd/csrc/recon_core.h) against it, a live run of the reference when its sources are
present, the drop-in header include/reconstruction.h, and the misuse cases of the C-ABI that need no device.

recon_core.h performs the reference's fp64 operations in the reference's order and is built here by the same
compiler family without FMA contraction, so equality is the derived expectation: every outcome code equal and every
accepted point bit-equal as float32, no tolerance."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import helpers as H
import recon_ref as R

CORE_CHECK = os.path.join(H.ROOT, "tests", "recon", "recon_core_check.cpp")


@pytest.fixture(scope="module")
def Z():
    with np.load(R.GOLDEN) as z:
        return {k: z[k] for k in z.files}


def runs(Z):
    for name in Z["scene_names"]:
        for j, s in enumerate(Z["%s_settings" % name]):
            yield str(name), j, tuple(s)


def same_run(got, want, where):
    assert len(got) == len(want), where
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0], (where, k, "active tracks")
        assert np.array_equal(g[2], w[2]), (where, k, "outcome codes")
        assert g[1].shape == w[1].shape and g[1].tobytes() == w[1].tobytes(), (where, k, "appended points")


def test_fixture_holds_every_outcome_and_stays_small(Z):
    assert os.path.getsize(R.GOLDEN) <= 1024 * 1024
    assert list(Z["scene_names"]) == ["frames", "synth", "edge"]
    seen = np.zeros(7, np.int64)
    for name, j, s in runs(Z):
        assert s == tuple(float(x) for x in R.SETTINGS[name][j])
        res = R.unpack_result(Z, "%s_%d" % (name, j))
        assert len(res) == len(Z["%s_n" % name])
        for active, pts, codes in res:
            seen += np.bincount(codes, minlength=7)
            assert len(pts) == int((codes == R.ACCEPTED).sum()) and np.isfinite(pts).all()
    assert (seen > 0).all(), dict(zip(R.CODE_NAMES, seen.tolist()))
    edge = R.unpack_scene(Z, "edge")
    assert len(edge[10][1]) == 0 and len(edge[3][1]) != len(np.unique(edge[3][1]["i1p"]))   # empty update, duplicate i1p
    assert np.array_equal(edge[5][0], np.eye(4))                                             # two identical poses
    assert Z["edge_0_nlost"][86] >= 30                                                       # the 76-frame tracks end here


def test_recon_core_reproduces_reference(Z, tmp_path):
    """recon_core.h built by g++ -ffp-contract=off, its SVD scratch contiguous (S = 1) and interleaved as in LDS
    (S = 64): active tracks, every outcome code and every appended point equal the reference's, bit for bit"""
    exe = str(tmp_path / "recon_core_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe, CORE_CHECK])
    for name in Z["scene_names"]:
        scene = R.unpack_scene(Z, name)
        path = str(tmp_path / ("%s.bin" % name))
        R.write_scene(path, scene)
        for j, s in enumerate(Z["%s_settings" % name]):
            for S in (1, 64):
                b = subprocess.run([exe, path] + [repr(float(c)) for c in Z["calib"]] + R.setting_args(s) + [str(S)],
                                   check=True, capture_output=True).stdout
                got = R.parse_run(b, len(scene))
                same_run(got, R.unpack_result(Z, "%s_%d" % (name, j)), (name, j, S))


@pytest.mark.skipif(not R.have_ref(), reason="the reference's sources are not on this machine")
def test_live_reference_equals_goldens(Z):
    with tempfile.TemporaryDirectory() as tmp:
        exe = R.build_harness(tmp)
        for name in Z["scene_names"]:
            scene = R.unpack_scene(Z, name)
            path = os.path.join(tmp, "%s.bin" % name)
            R.write_scene(path, scene)
            for j, s in enumerate(Z["%s_settings" % name]):
                got = R.run_scene(exe, path, len(scene), s, tuple(Z["calib"]))
                same_run(got, R.unpack_result(Z, "%s_%d" % (name, j)), (name, j))
        # the synthetic scenes are what recon_ref generates today
        for name, scene in (("synth", R.synth_scene()), ("edge", R.edge_scene())):
            for (T, m), (gT, gm) in zip(scene, R.unpack_scene(Z, name)):
                assert np.array_equal(T, gT) and m.tobytes() == gm.tobytes(), name


def test_dropin_compiles_against_include_alone(tmp_path):
    """demo_structure_from_motion.m's loop written against libviso2/src/reconstruction.h compiles with include/ only"""
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-I" + os.path.join(H.ROOT, "include"), "-c",
                           os.path.join(H.ROOT, "tests", "recon", "recon_dropin.cpp"), "-o", str(tmp_path / "d.o")])


def test_misuse_is_refused_without_a_device():
    """update before setCalibration and a second setCalibration return SVH_ERR_BAD_ARG before anything touches the
    device; the getters of a fresh object answer 0"""
    import svhip as S
    L = S.lib()
    L.svh_recon_create.restype = C.c_void_p
    L.svh_recon_destroy.argtypes = [C.c_void_p]
    L.svh_recon_set_calibration.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double]
    L.svh_recon_update.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_double,
                                   C.c_double]
    L.svh_recon_num_points.argtypes = [C.c_void_p]
    L.svh_recon_num_tracks.argtypes = [C.c_void_p]
    r = L.svh_recon_create()
    assert r
    Tr = np.eye(4)
    m = np.zeros(1, S.P_MATCH)
    assert L.svh_recon_update(r, None, 0, Tr.ctypes.data, 1, 2, 30.0, 2.0) == S.ERR_BAD_ARG
    assert L.svh_recon_set_calibration(r, 645.2, 635.9, 194.1) == S.OK
    assert L.svh_recon_set_calibration(r, 645.2, 635.9, 194.1) == S.ERR_BAD_ARG
    assert L.svh_recon_update(r, None, 0, None, 1, 2, 30.0, 2.0) == S.ERR_BAD_ARG       # no Tr
    assert L.svh_recon_update(r, None, 3, Tr.ctypes.data, 1, 2, 30.0, 2.0) == S.ERR_BAD_ARG   # matches missing
    m["i1p"] = -1
    assert L.svh_recon_update(r, m.ctypes.data, 1, Tr.ctypes.data, 1, 2, 30.0, 2.0) == S.ERR_BAD_ARG
    assert L.svh_recon_num_points(r) == 0 and L.svh_recon_num_tracks(r) == 0
    L.svh_recon_destroy(r)
