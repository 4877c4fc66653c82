"""GPU parity of Reconstruction (svh_recon_* C-ABI; k_recon_tracks and k_recon_compact in recon_kernels.hip) against
the reference's own output in tests/golden/recon.npz (make_goldens_recon.py).  Only the fixture and
tests/golden/full/ are read.

Per update of every scene and setting the number of active tracks, the outcome code of every lost track and the
number and order of the appended points must be identical.  Coordinates: the device's fp64 + - * / sqrt are correctly
rounded and acos feeds a comparison only, so bit-equal float32 is expected and that is what is measured (the largest
deviation is printed).  The bound, should the device differ, is the reference's own convergence step 1e-5 plus one
float32 ulp of the coordinate; a flipped outcome code is a failure."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import recon_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Z():
    with np.load(R.GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def S():
    import svhip
    return svhip


def runs(Z):
    return [(str(name), j) for name in Z["scene_names"] for j in range(len(Z["%s_settings" % name]))]


class Runner:
    """one svhip.Reconstruction fed the fixture's matches and motion, one update per step"""

    def __init__(self, S, Z, name, j):
        self.rec = S.Reconstruction()
        self.rec.set_calibration(*[float(c) for c in Z["calib"]])
        self.scene = R.unpack_scene(Z, name)
        self.s = Z["%s_settings" % name][j]
        self.want = R.unpack_result(Z, "%s_%d" % (name, j))
        self.k, self.where, self.worst = 0, (name, j), 0.0

    def step(self):
        Tr, m = self.scene[self.k]
        before = self.rec.num_points()
        self.rec.update(R.to_p_match(m), Tr, int(self.s[0]), int(self.s[1]), float(self.s[2]), float(self.s[3]))
        active, pts, codes = self.want[self.k]
        where = self.where + (self.k,)
        assert self.rec.num_tracks() == active, where
        got_codes, got_xyz = self.rec.outcomes()
        assert np.array_equal(got_codes, codes), (where, np.flatnonzero(got_codes != codes)[:10])
        got = got_xyz[got_codes == R.ACCEPTED]
        assert self.rec.num_points() == before + len(pts), where
        assert got.shape == pts.shape, where
        if len(pts):
            dev = np.abs(got.astype(np.float64) - pts.astype(np.float64))
            self.worst = max(self.worst, float(dev.max()))
            assert (dev <= 1e-5 + np.spacing(np.abs(pts)).astype(np.float64)).all(), (where, dev.max())
        self.k += 1
        return got

    def run(self):
        out = [self.step() for _ in range(len(self.scene))]
        return np.concatenate(out) if out else np.zeros((0, 3), np.float32)


def test_every_scene_and_setting_matches_reference(S, Z):
    worst = 0.0
    for name, j in runs(Z):
        run = Runner(S, Z, name, j)
        accepted = run.run()
        worst = max(worst, run.worst)
        # get_points is the concatenation of the accepted outcomes, in order
        pts = run.rec.points()
        assert pts.tobytes() == accepted.tobytes(), (name, j)
        assert pts.shape == Z["%s_%d_points" % (name, j)].shape
        print("recon %s setting %d: %d points, largest coordinate deviation %.3g" % (name, j, len(pts), run.worst))
        run.rec.close()
    print("largest coordinate deviation over all scenes: %.3g" % worst)
    # measured on an MI355X: 0 -- every coordinate bit-equal; the derived expectation is asserted from here on
    assert worst == 0.0, "the device's points are within the bound but no longer bit-equal to the reference's"


def test_resident_points_hold_the_same_bytes(S, Z):
    run = Runner(S, Z, "synth", 0)
    run.run()
    pts = run.rec.points()
    addr, n = run.rec.points_device()
    assert n == len(pts) and n > 0 and addr
    # read the resident array with the HIP runtime the library is linked against
    hip_memcpy = S.lib().hipMemcpy
    hip_memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    back = np.zeros((n, 3), np.float32)
    assert hip_memcpy(back.ctypes.data, addr, 12 * n, 2) == 0   # hipMemcpyDeviceToHost
    assert back.tobytes() == pts.tobytes() == Z["synth_0_points"].tobytes()


def test_two_objects_interleaved(S, Z):
    a, b = Runner(S, Z, "synth", 1), Runner(S, Z, "edge", 0)
    for k in range(max(len(a.scene), len(b.scene))):
        if k < len(a.scene):
            a.step()
        if k < len(b.scene):
            b.step()
    assert a.rec.points().tobytes() == Z["synth_1_points"].tobytes()
    assert b.rec.points().tobytes() == Z["edge_0_points"].tobytes()


def test_object_works_after_refused_calls(S, Z):
    rec = S.Reconstruction()
    with pytest.raises(S.SvhError) as e:
        rec.update(np.zeros(0, S.P_MATCH), np.eye(4))            # before set_calibration
    assert e.value.code == S.ERR_BAD_ARG
    run = Runner(S, Z, "edge", 1)
    run.rec.close()
    run.rec = rec
    rec.set_calibration(*[float(c) for c in Z["calib"]])
    for k in range(len(run.scene)):
        if k in (2, 9, 40):
            with pytest.raises(S.SvhError) as e:
                rec.set_calibration(1.0, 2.0, 3.0)               # a second calibration
            assert e.value.code == S.ERR_BAD_ARG
            bad = np.zeros(2, S.P_MATCH)
            bad["i1p"] = -5
            with pytest.raises(S.SvhError) as e:
                rec.update(bad, np.eye(4))
            assert e.value.code == S.ERR_BAD_ARG
        run.step()
    assert len(rec.points()) == len(Z["edge_1_points"])


def test_failed_allocation_leaves_the_object_usable(S, Z):
    """an allocation that fails before the tracks are touched, a launch check that fails before the wait and one
    that fails after it: SVH_ERR_HIP, nothing changed, and the same update given again continues the reference's
    run"""
    L = S.lib()
    L.svh_test_fail_at.argtypes = [C.c_char_p]
    run = Runner(S, Z, "synth", 1)
    failures = 0
    try:
        for k in range(len(run.scene)):
            if k in (0, 3, 17):
                tracks, points = run.rec.num_tracks(), run.rec.num_points()
                L.svh_test_fail_at(b"malloc:1:1" if k == 0 else (b"launch:1:1" if k == 3 else b"launch:2:1"))
                Tr, m = run.scene[k]
                with pytest.raises(S.SvhError) as e:
                    run.rec.update(R.to_p_match(m), Tr)
                L.svh_test_fail_at(b"")
                assert e.value.code == S.ERR_HIP
                assert (run.rec.num_tracks(), run.rec.num_points()) == (tracks, points)
                failures += 1
            run.step()
    finally:
        L.svh_test_fail_at(b"")
    assert failures == 3 and len(run.rec.points()) == len(Z["synth_1_points"])


def test_timing_entries(S, Z):
    run = Runner(S, Z, "synth", 0)
    run.rec.set_timing(True)
    for _ in range(5):
        run.step()
    ms = run.rec.timing()
    assert ms.shape == (3,) and (ms >= 0).all() and ms[1] > 0


def test_dropin_runs_demo_loop(Z, tmp_path):
    """the C++ drop-in (include/reconstruction.h + include/viso_mono.h, demo_structure_from_motion.m's loop) runs
    the seven frames.  Its matches are the reference's and its motion agrees within 1e-9 (test_vo_mono_gpu.py), so
    the point count is the fixture's up to tracks that sit on a threshold: within a factor of two of it."""
    import mono_ref
    exe = str(tmp_path / "recon_dropin")
    lib = os.path.join(H.ROOT, "stereo-vision_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-I" + os.path.join(H.ROOT, "include"), "-o", exe,
                           os.path.join(H.ROOT, "tests", "recon", "recon_dropin.cpp"), "-L" + lib, "-lsvhip",
                           "-Wl,-rpath," + lib])
    mono_ref.write_frames(str(tmp_path))
    out = subprocess.run([exe, str(tmp_path)] + R.setting_args(Z["frames_settings"][0]), check=True,
                         capture_output=True, text=True).stdout
    print(out)
    lines = out.strip().splitlines()
    assert len(lines) == 7 and lines[-1].startswith("points ")
    n, want = int(lines[-1].split()[1]), len(Z["frames_0_points"])
    assert want > 0 and want / 2 <= n <= 2 * want, (n, want)
