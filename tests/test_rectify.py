"""CPU: the rectification arithmetic (include/svh_rectify.h).  OpenCV is not available, so nothing here compares against
the reference's cv::initUndistortRectifyMap / cv::remap; the contract is the arithmetic the header states, pinned by

  * known answers derived by hand (identity, integer and half-pixel shifts, the ties of the rounding, a row with W = 0),
  * an independent round trip of the KITTI-like rig's maps (undistort by iteration, rotate, project),
  * bit-equality of the C++ core (stereo-vision_amd/csrc/rectify_core.h, compiled on the spot with -ffp-contract=off)
    with the numpy restatement tests/rectify_ref.py, which also produced tests/golden/rectify.npz.  Both sides perform
    the same IEEE operations in the same order, so equality is the derived expectation: maps as bit patterns, images
    byte for byte, no tolerance.

Plus svh_rectify_from_kitti, the misuse cases of the C-ABI that need no device, and svh_rectify_get_maps."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import rectify_ref as R

CORE_CHECK = os.path.join(H.ROOT, "tests", "rectify", "rectify_core_check.cpp")


@pytest.fixture(scope="module")
def Z():
    return R.load_golden()


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    d = tmp_path_factory.mktemp("rectify_core")
    exe = str(d / "rectify_core_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe, CORE_CHECK])

    def run(cam, S, dw, dh, border, stride=None):
        job = str(d / "job.bin")
        R.write_job(job, cam, S, dw, dh, border, stride)
        return R.parse_run(subprocess.run([exe, job], check=True, capture_output=True).stdout, dw, dh)
    return run


@pytest.fixture(scope="module")
def rig_maps():
    """the full-size maps of the rig by the restatement, computed once: [(u, v, mx, my)] per camera"""
    out = []
    for cam in R.RIG:
        u, v = R.maps64(cam, *R.RIG_DST)
        with np.errstate(all="ignore"):
            out.append((u, v, u.astype(np.float32), v.astype(np.float32)))
    return out


def test_fixture_is_the_restatements_and_stays_small(Z):
    assert os.path.getsize(R.GOLDEN) <= 1048576 <= 2632349       # (the largest fixture committed: urban1_robotics.npz)
    assert "restatement" in str(Z["produced_by"]) and "NOT an OpenCV run" in str(Z["produced_by"])
    assert list(Z["hand_names"]) == [n for n, _ in R.hand_cases()]
    assert list(Z["shape_names"]) == [n for n, _ in R.shape_cases()]
    for k, (name, (cam, sw, sh, dw, dh)) in enumerate(R.shape_cases()):
        assert tuple(Z[name + "_size"]) == (sw, sh, dw, dh)
        assert R.same_bits(Z[name + "_src"], R.source(sw, sh, seed=k))
        mx, my = R.maps(cam, dw, dh)
        assert R.same_bits(Z[name + "_mx"], mx) and R.same_bits(Z[name + "_my"], my), name
        for border in (R.WRAP, R.ZERO):
            assert R.same_bits(Z["%s_out%d" % (name, border)], R.remap(Z[name + "_src"], mx, my, border)), name


def test_known_answers_derived_by_hand(Z):
    """what the fixture holds for the hand cases is what the formulas give on paper: D = 0, K = I, so the map is the
    output pixel moved by -(cx, cy), exactly representable; the sample weights follow from the fraction alone"""
    S = Z["hand_src"]
    h, w = S.shape
    assert len(set(S.ravel().tolist())) == w * h                  # distinct bytes: a wrong tap cannot hide
    i, j = np.mgrid[0:h, 0:w]
    s = S.astype(np.int64)

    def zero_shift(dy, dx):                                       # S[i + dy, j + dx], 0 outside
        out = np.zeros_like(s)
        out[:h - dy, :w - dx] = s[dy:, dx:]
        return out

    def maps_are(name, x, y):
        assert R.same_bits(Z[name + "_mx"], x.astype(np.float32)) and R.same_bits(Z[name + "_my"], y.astype(np.float32))

    maps_are("identity", j, i)
    assert np.array_equal(Z["identity_out0"], S) and np.array_equal(Z["identity_out1"], S)
    maps_are("shift", j + 3, i + 2)
    assert np.array_equal(Z["shift_out1"], zero_shift(2, 3))
    assert np.array_equal(Z["shift_out0"], np.roll(S, (-2, -3), (0, 1)))          # the cyclic shift
    maps_are("half", j + 0.5, i)
    assert np.array_equal(Z["half_out1"], (s + zero_shift(0, 1) + 1) >> 1)
    assert np.array_equal(Z["half_out0"], (s + np.roll(s, -1, 1) + 1) >> 1)
    assert np.array_equal(Z["half_out0"][:, :-1], ((s[:, :-1] + s[:, 1:] + 1) >> 1))
    maps_are("tie1", j + 1.0 / 64, i)                             # 32 j + 0.5 rounds to the even 32 j: fraction 0
    assert np.array_equal(Z["tie1_out0"], S) and np.array_equal(Z["tie1_out1"], S)
    maps_are("tie3", j + 3.0 / 64, i)                             # 32 j + 1.5 rounds to the even 32 j + 2: fraction 2/32
    assert np.array_equal(Z["tie3_out1"], (30 * 32 * s + 2 * 32 * zero_shift(0, 1) + 512) >> 10)
    assert np.array_equal(Z["tie3_out0"], (30 * 32 * s + 2 * 32 * np.roll(s, -1, 1) + 512) >> 10)
    # w0: W = (i - 1) / 2 vanishes on row 1, whose entries are not finite and give 0 in both modes
    assert not np.isfinite(Z["w0_mx"][1]).any() and not np.isfinite(Z["w0_my"][1]).any()
    assert np.isfinite(Z["w0_mx"][[0] + list(range(2, h))]).all()
    for border in (0, 1):
        assert not Z["w0_out%d" % border][1].any() and Z["w0_out%d" % border][2:].any()


def test_singular_projection_is_refused(core):
    import svhip  # noqa: F401
    from svhip import rectify as SR
    S = R.distinct_source(4, 4)
    for P in ([[1, 0, 0, 0], [2, 0, 0, 0], [0, 0, 1, 0]], np.zeros((3, 4)), [[np.inf, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]],
              [[np.nan, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]]):
        cam = R.camera(P=P)
        assert R.inverse_pr(cam) is None
        assert core(cam, S, 4, 4, R.WRAP) is None
        with pytest.raises(SR.SvhError) as e:
            SR.Rectifier(SR.params((4, 4), (4, 4), [cam]))
        assert e.value.code == SR.ERR_BAD_ARG and "singular" in str(e.value)


def test_core_equals_fixture_on_hand_and_shape_cases(Z, core):
    """rectify_core.h built by g++ -ffp-contract=off: every case of the fixture, both border modes, rows packed and
    three bytes apart; everything identical"""
    cases = [(n, cam, Z["hand_src"], R.HAND_W, R.HAND_H) for n, cam in R.hand_cases()]
    cases += [(n, cam, Z[n + "_src"], dw, dh) for n, (cam, sw, sh, dw, dh) in R.shape_cases()]
    for name, cam, S, dw, dh in cases:
        for border in (R.WRAP, R.ZERO):
            for stride in (S.shape[1], S.shape[1] + 3):
                mx, my, out = core(cam, S, dw, dh, border, stride)
                assert R.same_bits(mx, Z[name + "_mx"]) and R.same_bits(my, Z[name + "_my"]), name
                assert R.same_bits(out, Z["%s_out%d" % (name, border)]), (name, border, stride)


def test_core_equals_restatement_on_the_rig(Z, core, rig_maps):
    """the KITTI-like rig at full size, 1392x512 -> 1242x375, both cameras and border modes"""
    for c, cam in enumerate(R.RIG):
        _, _, mx, my = rig_maps[c]
        S = R.source(*R.RIG_SRC, seed=c)
        assert R.same_bits(R.window(mx), Z["rig%d_mx" % c]) and R.same_bits(R.window(my), Z["rig%d_my" % c])
        for border in (R.WRAP, R.ZERO):
            gx, gy, out = core(cam, S, *R.RIG_DST, border)
            assert R.same_bits(gx, mx) and R.same_bits(gy, my), c
            want = R.remap(S, mx, my, border)
            assert R.same_bits(out, want), (c, border)
            assert R.same_bits(R.window(want), Z["rig%d_out%d" % (c, border)])


def test_round_trip_of_the_rig(rig_maps):
    """Independent of the forward formula: every map entry (in float64, before the cast) is undistorted by 20 rounds of
    fixed-point iteration of the distortion model, rotated by R and projected by P, and must come back within 1e-6
    pixels of the output pixel (j, i) it belongs to.  The bound is the condition the issue sets.  Observed with the
    restatement on the CPU: 8.53e-07 pixels for the left camera, 3.62e-07 for the right one -- what is left is the
    iteration's own convergence (30 rounds: 7.5e-11 and 2.0e-11), not the maps.  The float32 maps are the casts of
    these entries (test_core_equals_restatement_on_the_rig compares them bit for bit)."""
    i, j = np.mgrid[0:R.RIG_DST[1], 0:R.RIG_DST[0]]
    for c, cam in enumerate(R.RIG):
        u, v, mx, my = rig_maps[c]
        assert np.isfinite(u).all() and np.isfinite(v).all()
        jj, ii = R.round_trip(cam, u, v, rounds=20)
        err = max(np.abs(jj - j).max(), np.abs(ii - i).max())
        print("camera %d: round trip max error %.3e pixels" % (c, err))
        assert err <= 1e-6, (c, err)
        assert np.abs(mx - u).max() <= 2.0 ** -13 and np.abs(my - v).max() <= 2.0 ** -14    # half an ulp below 2048 / 1024


def rig_calib_text():
    """calib_cam_to_cam.txt in the layout tests/test_kitti_io.py writes, cameras 0 and 1 holding the rig"""
    shapes = (("S", 2), ("K", 9), ("D", 5), ("R", 9), ("T", 3), ("S_rect", 2), ("R_rect", 9), ("P_rect", 12))
    rng = np.random.default_rng(3)
    lines = ["calib_time: 09-Jan-2012 13:57:47", "corner_dist: 9.950000e-02"]
    for i in range(4):
        cam = R.RIG[i % 2]
        given = {"S": R.RIG_SRC if i < 2 else (1000.0, 400.0), "K": cam["K"].ravel(), "D": cam["D"],
                 "S_rect": R.RIG_DST, "R_rect": cam["R"].ravel(), "P_rect": cam["P"].ravel()}
        for name, n in shapes:
            vals = np.asarray(given.get(name, rng.normal(0, 1, n)), np.float64)
            lines.append("%s_0%d: " % (name, i) + " ".join("%.6e" % v for v in vals))
    return "\n".join(lines) + "\n"


def test_params_from_kitti(tmp_path):
    from svhip import kitti, rectify as SR
    p = str(tmp_path / "calib_cam_to_cam.txt")
    open(p, "w").write(rig_calib_text())
    calib = kitti.read_cam_to_cam(p)
    prm = SR.params_from_kitti(calib, 0, 1, SR.ZERO)
    assert (prm.src_width, prm.src_height, prm.dst_width, prm.dst_height) == R.RIG_SRC + R.RIG_DST
    assert (prm.border, prm.cameras) == (SR.ZERO, 2)
    def as_read(a):                          # the reader parses every value as float, as readCalibFileMatrix does
        return np.asarray(a, np.float64).ravel().astype(np.float32).astype(np.float64)

    for c in range(2):
        for name in ("K", "D", "R", "P"):
            assert np.array_equal(np.array(getattr(prm.cam[c], name)[:]), as_read(R.RIG[c][name])), (c, name)
    one = SR.params_from_kitti(calib, 1, -1)
    assert (one.cameras, one.border) == (1, SR.WRAP)
    assert np.array_equal(np.array(one.cam[0].K[:]), as_read(R.RIG[1]["K"]))
    # an object made from them answers with the maps of the camera as it was read
    r = SR.Rectifier(one)
    u, v = R.maps(R.camera(**{k: as_read(a) for k, a in R.RIG[1].items()}), *R.RIG_DST)
    mx, my = r.maps(0)
    assert R.same_bits(mx, u) and R.same_bits(my, v)
    r.close()
    for bad in ((4, 1, 0), (0, 4, 0), (-1, 1, 0), (0, -2, 0), (0, 1, 2), (0, 2, 0)):   # (camera 2 differs in size)
        with pytest.raises(SR.SvhError) as e:
            SR.params_from_kitti(calib, *bad)
        assert e.value.code == SR.ERR_BAD_ARG
    calib.S_rect[0][0] = 1242.5
    with pytest.raises(SR.SvhError):
        SR.params_from_kitti(calib, 0, -1)


def test_defaults_and_misuse_without_a_device():
    import svhip as S
    from svhip import rectify as SR
    L = SR._bind()
    p = SR.default_params()
    assert (p.src_width, p.src_height, p.dst_width, p.dst_height, p.border, p.cameras) == (0, 0, 0, 0, SR.WRAP, 2)
    for c in range(2):
        assert list(p.cam[c].K) == list(np.eye(3).ravel()) == list(p.cam[c].R) and not any(p.cam[c].D)
        assert list(p.cam[c].P) == list(np.eye(3, 4).ravel())
    assert not L.svh_rectify_create(None)
    assert not L.svh_rectify_create(C.byref(p))                       # sizes not set
    cam = R.camera()
    for src, dst, cams, border in (((0, 4), (4, 4), [cam], 0), ((4, 4), (4, -1), [cam], 0), ((16385, 4), (4, 4), [cam], 0),
                                   ((4, 4), (4, 16385), [cam], 0), ((4, 4), (4, 4), [], 0), ((4, 4), (4, 4), [cam] * 3, 0),
                                   ((4, 4), (4, 4), [cam], 2)):
        with pytest.raises(SR.SvhError) as e:
            SR.Rectifier(SR.params(src, dst, cams, border))
        assert e.value.code == S.ERR_BAD_ARG
    SR.Rectifier(SR.params((16384, 1), (1, 16384), [cam])).close()    # the largest sides are accepted; creation is cheap
    r = SR.Rectifier(SR.params((8, 6), (5, 4), [cam]))
    src, dst = np.zeros((6, 8), np.uint8), np.full((4, 5), 7, np.uint8)
    bad = [(1, src.ctypes.data, 0, 8, dst.ctypes.data, 0, 5), (-1, src.ctypes.data, 0, 8, dst.ctypes.data, 0, 5),
           (0, None, 0, 8, dst.ctypes.data, 0, 5), (0, src.ctypes.data, 0, 8, None, 0, 5),
           (0, src.ctypes.data, 0, 7, dst.ctypes.data, 0, 5), (0, src.ctypes.data, 0, 8, dst.ctypes.data, 0, 4)]
    for args in bad:
        assert L.svh_rectify_remap(r._h, *args) == S.ERR_BAD_ARG, args
    assert L.svh_rectify_pairs_device(r._h, 1, 1, 1, 8, 48, 1, 1, 5, 20) == S.ERR_BAD_ARG      # one camera only
    assert L.svh_rectify_get_maps(r._h, 1, None, None, 0) == S.ERR_BAD_ARG
    assert L.svh_rectify_get_maps(r._h, 0, None, None, 0) == 20                                 # the size query
    two = SR.Rectifier(SR.params((8, 6), (5, 4), [cam, cam]))
    for args in ((0, 1, 1, 8, 48, 1, 1, 5, 20), (4097, 1, 1, 8, 48, 1, 1, 5, 20), (1, None, 1, 8, 48, 1, 1, 5, 20),
                 (1, 1, 1, 7, 48, 1, 1, 5, 20), (2, 1, 1, 8, 47, 1, 1, 5, 20), (2, 1, 1, 8, 48, 1, 1, 5, 19)):
        assert L.svh_rectify_pairs_device(two._h, *args) == S.ERR_BAD_ARG, args
    if S.device_count() == 0:                                          # there is no CPU fall-back for the compute entries
        assert L.svh_rectify_remap(r._h, 0, src.ctypes.data, 0, 8, dst.ctypes.data, 0, 5) == S.ERR_NO_DEVICE
        assert L.svh_rectify_pairs_device(two._h, 1, 1, 1, 8, 48, 1, 1, 5, 20) == S.ERR_NO_DEVICE
        assert (dst == 7).all()
    assert r.release() >= 0 and list(r.timing()) == [0, 0]
    r.close()
    two.close()
    L.svh_rectify_destroy(None)


def test_get_maps_equals_fixture(Z):
    """without a device the host form of the core answers; with one, k_rect_maps does: the same bits either way"""
    from svhip import rectify as SR
    for name, cam in R.hand_cases():
        r = SR.Rectifier(SR.params((R.HAND_W, R.HAND_H), (R.HAND_W, R.HAND_H), [cam, cam]))
        for c in range(2):
            mx, my = r.maps(c)
            assert R.same_bits(mx, Z[name + "_mx"]) and R.same_bits(my, Z[name + "_my"]), name
        r.close()
    for name, (cam, sw, sh, dw, dh) in R.shape_cases():
        r = SR.Rectifier(SR.params((sw, sh), (dw, dh), [cam]))
        mx, my = r.maps(0)
        assert R.same_bits(mx, Z[name + "_mx"]) and R.same_bits(my, Z[name + "_my"]), name
        r.close()
