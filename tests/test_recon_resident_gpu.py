"""GPU: Reconstruction with its track table resident in device memory (svh_recon_create_resident; the k_rt_* kernels
of recon_track_kernels.hip) against the reference's own record in tests/golden/recon.npz and
tests/golden/recon_shared.npz.  Only those fixtures are read.

recon.npz holds the case of two matches with the same i1p (scene edge, update 3) and of two matches with the same i1c
(update 6), but no later match reaches the feature index the two tracks then share.  Scene `shared` of
recon_shared.npz (make_goldens_recon_shared.py) has five updates in which one does: the higher-indexed track is
extended and the other is lost (k_rt_scatter's atomicMax), visible in the outcome codes and the points
(tests/test_recon_resident.py shows that the opposite rule does not reproduce that scene).  Every test below that
walks "every scene and setting" walks it too.

After EVERY update of every scene and setting the number of active tracks, the outcome code of every lost track in
order and the appended points as float32 bytes must equal the reference's.  No tolerance: the association is integer
work, and the lost tracks go through the same recon::track_outcome as on a host-table object, whose points are
bit-equal to the reference's (tests/test_recon_gpu.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers as H
import recon_ref as R

pytestmark = pytest.mark.gpu

SHARED = os.path.join(H.GOLDEN, "recon_shared.npz")


@pytest.fixture(scope="module")
def Z():
    """both fixtures as one: the scenes of recon.npz, then `shared`"""
    with np.load(R.GOLDEN) as z, np.load(SHARED) as y:
        out = {k: z[k] for k in z.files}
        assert np.array_equal(y["calib"], z["calib"])
        out.update({k: y[k] for k in y.files if k not in ("calib", "scene_names")})
        out["scene_names"] = np.concatenate([z["scene_names"], y["scene_names"]])
        return out


@pytest.fixture(scope="module")
def S():
    import svhip
    return svhip


def runs(Z):
    return [(str(name), j) for name in Z["scene_names"] for j in range(len(Z["%s_settings" % name]))]


class DeviceMatches:
    """svh_p_match records uploaded with the HIP runtime the library is linked against"""

    def __init__(self, S, m):
        L = S.lib()
        L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        L.hipFree.argtypes = [C.c_void_p]
        self.L, self.p, self.n = L, C.c_void_p(), len(m)
        assert L.hipMalloc(C.byref(self.p), max(m.nbytes, 16)) == 0
        if len(m):
            assert L.hipMemcpy(self.p, m.ctypes.data, m.nbytes, 1) == 0   # hipMemcpyHostToDevice

    def free(self):
        self.L.hipFree(self.p)


class Runner:
    """one svhip.Reconstruction fed the fixture's matches and motion, one update per step; every step is compared
    with the reference's record"""

    def __init__(self, S, Z, name, j, resident=True, how="host"):
        self.S = S
        self.rec = S.Reconstruction(resident=resident)
        self.rec.set_calibration(*[float(c) for c in Z["calib"]])
        self.scene = R.unpack_scene(Z, name)
        self.s = Z["%s_settings" % name][j]
        self.want = R.unpack_result(Z, "%s_%d" % (name, j))
        self.all = Z["%s_%d_points" % (name, j)]
        self.k, self.where, self.how = 0, (name, j), how

    def settings(self):
        return int(self.s[0]), int(self.s[1]), float(self.s[2]), float(self.s[3])

    def done(self):
        return self.k >= len(self.scene)

    def matches(self):
        return R.to_p_match(self.scene[self.k][1])

    def update(self):
        Tr, _ = self.scene[self.k]
        m = self.matches()
        if self.how == "host":
            self.rec.update(m, Tr, *self.settings())
        else:
            d = DeviceMatches(self.S, m)
            top = int(max(m["i1p"].max(), m["i1c"].max())) + 1 if len(m) else 0
            try:
                self.rec.update_device(d.p if len(m) else None, len(m), top, Tr, *self.settings())
            finally:
                d.free()

    def check(self, before):
        active, pts, codes = self.want[self.k]
        where = self.where + (self.k,)
        assert self.rec.num_tracks() == active, where
        got_codes, got_xyz = self.rec.outcomes()
        assert np.array_equal(got_codes, codes), (where, np.flatnonzero(got_codes != codes)[:10])
        got = got_xyz[got_codes == R.ACCEPTED]
        assert self.rec.num_points() == before + len(pts), where
        assert got.shape == pts.shape and got.tobytes() == pts.astype(np.float32).tobytes(), where
        self.k += 1

    def step(self):
        before = self.rec.num_points()
        self.update()
        self.check(before)

    def run(self):
        while not self.done():
            self.step()
        self.finish()

    def finish(self):
        pts = self.rec.points()
        assert pts.shape == self.all.shape and pts.tobytes() == self.all.tobytes(), self.where
        self.rec.close()


def test_every_scene_and_setting_matches_reference(S, Z):
    for name, j in runs(Z):
        Runner(S, Z, name, j).run()


def test_device_matches_every_scene_and_setting(S, Z):
    for name, j in runs(Z):
        Runner(S, Z, name, j, how="device").run()


def test_out_of_range_index_is_refused_on_the_device(S, Z):
    run = Runner(S, Z, "edge", 0, how="device")
    while not run.done():
        if run.k in (0, 4, 7, 30):
            m = run.matches()
            tracks, points = run.rec.num_tracks(), run.rec.num_points()
            if len(m) == 0:
                m = np.zeros(1, S.P_MATCH)
            top = int(max(m["i1p"].max(), m["i1c"].max())) + 1
            for field, value in (("i1p", top), ("i1c", top + 7), ("i1p", -1), ("i1c", -3)):
                bad = m.copy()
                bad[field][len(bad) // 2] = value
                d = DeviceMatches(S, bad)
                with pytest.raises(S.SvhError) as e:
                    run.rec.update_device(d.p, len(bad), top, run.scene[run.k][0], *run.settings())
                d.free()
                assert e.value.code == S.ERR_BAD_ARG
                assert (run.rec.num_tracks(), run.rec.num_points()) == (tracks, points)
        run.step()
    run.finish()


def batch_step(S, group):
    """one svh_recon_update_batch over `group` (same settings): runners that are done, or None entries, sit out"""
    objs = [g.rec for g in group]
    live = [not g.done() for g in group]
    ms = [g.matches() if ok else None for g, ok in zip(group, live)]
    Trs = [g.scene[g.k][0] if ok else None for g, ok in zip(group, live)]
    before = [g.rec.num_points() for g in group]
    tracks = [g.rec.num_tracks() for g in group]
    status = S.Reconstruction.update_batch(objs, ms, Trs, *group[0].settings())
    assert status == [0] * len(group)
    for g, ok, b, t in zip(group, live, before, tracks):
        if ok:
            g.check(b)
        else:
            assert (g.rec.num_points(), g.rec.num_tracks()) == (b, t)


def test_batch_of_different_scenes_and_settings(S, Z):
    """eleven objects, one per scene and setting, 87 updates for the longest: per step one call per setting (the
    settings are the call's), in which the objects of the other settings sit out, as do those whose scene has ended
    and, every fifth step, one more object whose update is then given on its own (svh_recon_update)."""
    all_runs = [Runner(S, Z, name, j) for name, j in runs(Z)]
    by_setting = {}
    for g in all_runs:
        by_setting.setdefault(g.settings(), []).append(g)
    assert len(by_setting) >= 4
    step = 0
    while not all(g.done() for g in all_runs):
        for setting, group in by_setting.items():
            # every object of every setting is handed to the call: those of other settings with NULL matches
            late = group[step % len(group)] if step % 5 == 4 else None
            objs = [g.rec for g in all_runs]
            live = [g in group and not g.done() and g is not late for g in all_runs]
            ms = [g.matches() if ok else None for g, ok in zip(all_runs, live)]
            Trs = [g.scene[g.k][0] if ok else None for g, ok in zip(all_runs, live)]
            before = [(g.rec.num_points(), g.rec.num_tracks()) for g in all_runs]
            status = S.Reconstruction.update_batch(objs, ms, Trs, *setting)
            assert status == [0] * len(all_runs)
            for g, ok, b in zip(all_runs, live, before):
                if ok:
                    g.check(b[0])
                else:
                    assert (g.rec.num_points(), g.rec.num_tracks()) == b
            if late is not None and not late.done():
                late.step()
        step += 1
    for g in all_runs:
        g.finish()


def test_batch_of_one_equals_single_call(S, Z):
    for name, j in (("synth", 1), ("edge", 1), ("shared", 2)):
        a, b = Runner(S, Z, name, j), Runner(S, Z, name, j)
        while not a.done():
            a.step()
            batch_step(S, [b])
            assert a.rec.outcomes()[0].tobytes() == b.rec.outcomes()[0].tobytes()
            assert a.rec.outcomes()[1].tobytes() == b.rec.outcomes()[1].tobytes()
        a.finish()
        b.finish()


def test_batch_status_is_per_object(S, Z):
    """an object whose matches are refused sits out with its own status; the others are updated"""
    a, b = Runner(S, Z, "synth", 0), Runner(S, Z, "synth", 0)
    for _ in range(3):
        batch_step(S, [a, b])
    bad = b.matches()
    bad["i1c"][0] = -2
    before = (b.rec.num_points(), b.rec.num_tracks())
    pts = a.rec.num_points()
    status = S.Reconstruction.update_batch([a.rec, b.rec], [a.matches(), bad], [a.scene[a.k][0]] * 2, *a.settings())
    assert status == [0, S.ERR_BAD_ARG]
    a.check(pts)
    assert (b.rec.num_points(), b.rec.num_tracks()) == before
    b.step()
    while not a.done():
        batch_step(S, [a, b])
    a.finish()
    b.finish()


FAULTS = [b"malloc:1:1", b"launch:1:1", b"wait:1:1", b"launch:2:1", b"copy:1:1"]


def test_injected_failure_leaves_the_object_as_it_was(S, Z):
    """an allocation that fails before anything is touched, the launch check, the wait, the check after the wait and
    the copy of the job table: SVH_ERR_HIP, nothing changed, and the same update given again continues the
    reference's run"""
    L = S.lib()
    L.svh_test_fail_at.argtypes = [C.c_char_p]
    run = Runner(S, Z, "synth", 1)
    at = dict(zip((0, 3, 9, 17, 25), FAULTS))
    failures = 0
    try:
        while not run.done():
            if run.k in at:
                tracks, points = run.rec.num_tracks(), run.rec.num_points()
                L.svh_test_fail_at(at[run.k])
                with pytest.raises(S.SvhError) as e:
                    run.update()
                L.svh_test_fail_at(b"")
                assert e.value.code == S.ERR_HIP, at[run.k]
                assert (run.rec.num_tracks(), run.rec.num_points()) == (tracks, points)
                failures += 1
            run.step()
    finally:
        L.svh_test_fail_at(b"")
    assert failures == len(FAULTS)
    run.finish()


def test_injected_failure_in_a_batch_leaves_every_object_as_it_was(S, Z):
    L = S.lib()
    L.svh_test_fail_at.argtypes = [C.c_char_p]
    group = [Runner(S, Z, "synth", 1), Runner(S, Z, "synth", 1), Runner(S, Z, "synth", 1)]
    at = dict(zip((0, 2, 8, 15, 22), FAULTS))
    failures = 0
    try:
        while not group[0].done():
            k = group[0].k
            if k in at:
                state = [(g.rec.num_tracks(), g.rec.num_points()) for g in group]
                L.svh_test_fail_at(at[k])
                with pytest.raises(S.SvhError) as e:
                    S.Reconstruction.update_batch([g.rec for g in group], [g.matches() for g in group],
                                                  [g.scene[g.k][0] for g in group], *group[0].settings())
                L.svh_test_fail_at(b"")
                assert e.value.code == S.ERR_HIP, at[k]
                assert [(g.rec.num_tracks(), g.rec.num_points()) for g in group] == state
                failures += 1
            batch_step(S, group)
    finally:
        L.svh_test_fail_at(b"")
    assert failures == len(FAULTS)
    for g in group:
        g.finish()


def test_host_table_and_resident_objects_interleaved(S, Z):
    a, b = Runner(S, Z, "synth", 2, resident=False), Runner(S, Z, "edge", 0, resident=True)
    c, d = Runner(S, Z, "edge", 0, resident=False), Runner(S, Z, "synth", 2, resident=True)
    e, f = Runner(S, Z, "shared", 1, resident=False), Runner(S, Z, "shared", 1, resident=True)
    group = [a, b, c, d, e, f]
    while not all(g.done() for g in group):
        for g in group:
            if not g.done():
                g.step()
    for g in group:
        g.finish()


def test_empty_first_update(S, Z):
    """update() with no matches on an object that has no tracks yet, alone and in a batch: nothing to do, no error"""
    a, b = S.Reconstruction(resident=True), S.Reconstruction(resident=True)
    for r in (a, b):
        r.set_calibration(*[float(c) for c in Z["calib"]])
    a.update(np.zeros(0, S.P_MATCH), np.eye(4))
    assert S.Reconstruction.update_batch([a, b], [np.zeros(0, S.P_MATCH)] * 2, [np.eye(4)] * 2) == [0, 0]
    for r in (a, b):
        assert (r.num_tracks(), r.num_points(), len(r.outcomes()[0])) == (0, 0, 0)
        r.close()


def test_getters_of_a_resident_object(S, Z):
    run = Runner(S, Z, "synth", 0)
    run.rec.set_timing(True)
    for _ in range(6):
        run.step()
    ms = run.rec.timing()
    assert ms.shape == (3,) and (ms >= 0).all() and ms[1] > 0
    pts = run.rec.points()
    addr, n = run.rec.points_device()
    assert n == len(pts) and n > 0 and addr
    hip_memcpy = S.lib().hipMemcpy
    hip_memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    back = np.zeros((n, 3), np.float32)
    assert hip_memcpy(back.ctypes.data, addr, 12 * n, 2) == 0   # hipMemcpyDeviceToHost
    assert back.tobytes() == pts.tobytes()
    run.rec.close()
