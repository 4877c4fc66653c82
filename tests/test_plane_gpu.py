"""GPU parity of PlaneEstimation (svh_plane_* C-ABI; k_plane_grid, k_plane_fit, k_plane_vote, k_plane_select in
plane_kernels.hip) against the reference's own output in tests/golden/plane.npz (make_goldens_plane.py).  Only
committed fixtures are read.

Required equal: the status, the list (length and contents), the draws every hypothesis consumed, every hypothesis'
vote, the winner and its inlier indices.  The per-hypothesis planes and _plane_d, _plane_e, _H are compared as bit
patterns: every operation behind them is an IEEE add / mul / div / sqrt in a fixed order (the device's fp64 forms are
correctly rounded, nothing is contracted), and the final refit, planeDsiTo3d and atan2 run on the host.  No
tolerance is used anywhere in this file."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import helpers as H
import plane_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Z():
    return R.load_golden()


@pytest.fixture(scope="module")
def S():
    import svhip
    return svhip


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


class DevMap:
    """a host array copied to device memory through the HIP runtime the library links"""

    def __init__(self, hip, a):
        self.hip, self.p = hip, C.c_void_p()
        a = np.ascontiguousarray(a)
        assert hip.hipMalloc(C.byref(self.p), C.c_size_t(max(a.nbytes, 16))) == 0
        assert hip.hipMemcpy(self.p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0   # HostToDevice
        self.addr = self.p.value

    def free(self):
        if self.p:
            self.hip.hipFree(self.p)
            self.p = None


def run_case(pl, calls, hip=None):
    """the calls of a case on one object, from host maps (hip None) or device-resident copies; the last status"""
    rc = None
    for D, width, seed in calls:
        if hip is None:
            rc = pl.estimate(D, width=width, seed=seed)
        else:
            d = DevMap(hip, D)
            try:
                rc = pl.estimate(d.addr, width=width, height=D.shape[0], step=D.shape[1], seed=seed)
            finally:
                d.free()
    return rc


def got_of(pl, rc):
    g = pl.taps()
    g["status"] = rc
    return g


def test_every_case_from_host_and_device_maps(S, Z, hip):
    for name, calls in R.cases():
        want = R.unpack_result(Z, name)
        for where in (None, hip):
            pl = S.PlaneEstimation()
            rc = run_case(pl, calls, where)
            R.same_result(got_of(pl, rc), want, (name, "host" if where is None else "device"))
            pl.close()


def urban_jobs():
    return [(name, seed) for name in R.URBAN for seed in (0, 2, 12345)]


@pytest.mark.parametrize("n", [4, 12])
def test_batch_equals_single_calls(S, Z, hip, n):
    jobs = [(name, 2) for name in R.URBAN] if n == 4 else urban_jobs()
    maps = {name: DevMap(hip, R.urban_d1(name)) for name in R.URBAN}
    objs = [S.PlaneEstimation() for _ in jobs]
    try:
        st = S.PlaneEstimation.estimate_batch(objs, [maps[name].addr for name, _ in jobs], R.W, R.HGT, R.W,
                                              seeds=[seed for _, seed in jobs])
        for (name, seed), o, rc in zip(jobs, objs, st):
            R.same_result(got_of(o, rc), R.unpack_result(Z, "%s_s%d" % (name, seed)), ("batch", n, name, seed))
    finally:
        for m in maps.values():
            m.free()
        for o in objs:
            o.close()


def test_straight_from_the_map_elas_left_on_the_device(S, Z, hip):
    """svh_elas_process_batch_device writes D1 to device memory; svh_plane_estimate reads it there"""
    for name in R.URBAN:
        with np.load(os.path.join(H.GOLDEN, name + ".npz")) as z:
            prm = H.ElasParams.from_buffer_copy(z["params"].tobytes())
            l, r = H.golden_pair(str(z["crop"]))
        h, w = l.shape
        assert (w, h) == (R.W, R.HGT)
        n = w * h
        dI1, dI2 = DevMap(hip, l), DevMap(hip, r)
        dD1, dD2 = DevMap(hip, np.zeros(n, np.float32)), DevMap(hip, np.zeros(n, np.float32))
        pl = S.PlaneEstimation()
        try:
            st = S.Elas(prm).process_batch_device(1, dI1.addr, dI2.addr, n, dD1.addr, dD2.addr, 4 * n, w, h, w)
            assert st == [0]
            for seed in (0, 2, 12345):
                rc = pl.estimate(dD1.addr, width=w, height=h, step=w, seed=seed)
                R.same_result(got_of(pl, rc), R.unpack_result(Z, "%s_s%d" % (name, seed)), ("elas", name, seed))
        finally:
            pl.close()
            for d in (dI1, dI2, dD1, dD2):
                d.free()


def test_non_default_parameters_match_the_host_core(S, tmp_path):
    """a 621x187 map with step_size 3, min_dist 25 and 1000 samples against plane_core.h on the host"""
    exe = str(tmp_path / "plane_core_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe,
                           os.path.join(H.ROOT, "tests", "plane", "plane_core_check.cpp")])
    D = R.half_map("urban2_stereomapper")
    assert D.shape == (187, 621)
    path = str(tmp_path / "job.bin")
    R.write_job(path, [(D, 621, 5)])
    want = R.parse_run(subprocess.run([exe, path, "1000", "3", "25", "1000"], check=True,
                                      capture_output=True).stdout, 1)[0]
    assert want["status"] == R.OK and len(want["votes"]) == 1000 and len(want["list"]) > 4000
    pl = S.PlaneEstimation(num_samples=1000, step_size=3, min_dist=25.0)
    rc = pl.estimate(D, width=621, seed=5)
    got = got_of(pl, rc)
    assert rc == want["status"]
    for k in ("list", "draws", "votes", "inliers"):
        assert np.array_equal(got[k], want[k]), k
    assert got["best"] == want["best"]
    for k in ("planes", "plane_d", "plane_e", "H"):
        assert np.ascontiguousarray(got[k], np.float64).tobytes() == want[k].tobytes(), k
    assert np.float32(got["pitch"]).tobytes() == np.float32(want["pitch"]).tobytes()
    pl.close()


def test_empty_map_returns_no_points_and_the_outputs_of_step_1(S, Z, hip):
    """the reference divides by zero here (rand() % 0); the library returns a status.  _pitch is kept."""
    pl = S.PlaneEstimation()
    road = R.unpack_result(Z, "urban2_stereomapper_s2")
    assert pl.estimate(R.urban_d1("urban2_stereomapper"), seed=2) == S.OK
    assert pl.pitch().tobytes() == road["pitch"].tobytes()
    for D in (np.zeros((120, 200), np.float32), np.full((120, 200), 0.5, np.float32)):
        for where in ("host", "device"):
            if where == "host":
                rc = pl.estimate(D, seed=3)
            else:
                d = DevMap(hip, D)
                rc = pl.estimate(d.addr, width=200, height=120, step=200, seed=3)
                d.free()
            assert rc == S.PLANE_NO_POINTS
            g = pl.taps()
            assert not g["plane_d"].any() and not g["plane_e"].any() and np.array_equal(g["H"], np.eye(4))
            assert g["pitch"].tobytes() == road["pitch"].tobytes()
            assert len(g["list"]) == 0 and len(g["votes"]) == 0 and g["best"] == -1 and len(g["inliers"]) == 0
    pl.close()


def test_injected_hip_failure_leaves_the_object_unchanged(S, Z):
    """the n-th HIP call of a kind returns an error code on the host (svh_test_fail_at, csrc/svh_internal.h); nothing
    faults on the device.  SVH_ERR_HIP, the object -- _pitch and taps included -- is what it was, the next call exact."""
    L = S.lib()
    L.svh_test_fail_at.argtypes = [C.c_char_p]
    pl = S.PlaneEstimation()
    first = R.unpack_result(Z, "urban1_robotics_s0")
    rc = pl.estimate(R.urban_d1("urban1_robotics"), seed=0)
    R.same_result(got_of(pl, rc), first, "before the failures")
    D = R.urban_d1("urban4_kitti")
    failures = 0
    try:
        # the buffers exist already: copies, launch checks and waits are what can fail
        for spec in (b"copy:1:1", b"copy:3:1", b"launch:1:1", b"launch:2:1", b"wait:1:1", b"wait:2:1", b"copy:5:1"):
            L.svh_test_fail_at(spec)
            with pytest.raises(S.SvhError) as e:
                pl.estimate(D, seed=12345)
            L.svh_test_fail_at(b"")
            assert e.value.code == S.ERR_HIP, spec
            R.same_result(got_of(pl, rc), first, ("after", spec))
            failures += 1
        pl.release()                                   # the next call has to allocate: that can fail too
        L.svh_test_fail_at(b"malloc:2:1")
        with pytest.raises(S.SvhError) as e:
            pl.estimate(D, seed=12345)
        L.svh_test_fail_at(b"")
        assert e.value.code == S.ERR_HIP
        R.same_result(got_of(pl, rc), first, "after malloc:2:1")
        failures += 1
    finally:
        L.svh_test_fail_at(b"")
    assert failures == 8
    rc = pl.estimate(D, seed=12345)
    R.same_result(got_of(pl, rc), R.unpack_result(Z, "urban4_kitti_s12345"), "after the failures")
    pl.close()


def test_two_objects_from_two_threads(S, Z):
    jobs = [("urban1_robotics", 2), ("urban3_kitti", 12345)]
    maps = [R.urban_d1(name) for name, _ in jobs]
    out, err = [None, None], []

    def work(k):
        try:
            pl = S.PlaneEstimation()
            for _ in range(4):
                rc = pl.estimate(maps[k], seed=jobs[k][1])
                out[k] = got_of(pl, rc)
            pl.close()
        except Exception as ex:   # noqa: BLE001
            err.append(ex)

    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not err, err
    for k, (name, seed) in enumerate(jobs):
        R.same_result(out[k], R.unpack_result(Z, "%s_s%d" % (name, seed)), ("thread", k))


def test_timing_and_release(S):
    pl = S.PlaneEstimation()
    pl.set_timing(True)
    D = R.urban_d1("urban2_stereomapper")
    for _ in range(3):
        assert pl.estimate(D, seed=2) == S.OK
    ms = pl.timing()
    assert ms.shape == (7,) and (ms >= 0).all() and ms[4] > 0 and ms[5] > 0 and ms[6] > 0
    assert ms[4] >= ms[0] + ms[1] + ms[2] + ms[3] - 1e-6
    d = pl.plane_dsi()
    assert pl.release() > 0
    assert np.array_equal(pl.plane_dsi(), d)
    assert pl.estimate(D, seed=2) == S.OK and np.array_equal(pl.plane_dsi(), d)
    pl.close()
