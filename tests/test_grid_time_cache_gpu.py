"""GPU: the TIME_STATIC and TIME bits of the engine's `valid` mask (stereo-vision_amd/csrc/grid_engine.cpp) pinned from outside,
against the tables of tests/grid_time_cache_cases.py, which tests/test_grid_time_cache.py pins on the CPU.

The rule under test is that of tests/test_grid_cache_gpu.py: a read through a cache is indistinguishable from a read computed from
the state as it is.  After every mutator of the grid -- those of every other layer, of the objects, of the prediction, of the pose
planner and of the archive included -- and after the layer's own setter, RCOST, RPOT, TPOT, TDIR, the statistics and a path are
compared with a fresh object that replays the history and is read once (tests/test_grid_time_gpu.py compares the object with the
header); an output
that the documented rule keeps is served under the simulated error launch:1:0, that is without a launch: no new computation.  The
other way round, the layer's setter and reads leave every other cached output current.  Every comparison is of bytes and exact.  The
window is the scene's 33 x 17."""
import ctypes as C

import pytest

import grid_cache_cases as CC
import grid_obj_cache_cases as OCC
import grid_pose_cache_cases as QCC
import grid_pred_cache_cases as PCC
import grid_time_cache_cases as TCC
import helpers as H   # puts the package on the path

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import svhip
    from svhip import grid
    assert svhip.device_count() > 0, "no HIP device: the product has no CPU fallback"
    svhip.lib().svh_test_fail_at.argtypes = [C.c_char_p]
    grid._bind()
    return grid


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


@pytest.fixture(autouse=True)
def restore(G):
    yield
    G.lib().svh_test_fail_at(None)


def served(G, g, names, before, why):
    """the outputs `names` are read without a launch and are what they were"""
    G.lib().svh_test_fail_at(b"launch:1:0")
    for n in names:
        try:
            got = TCC.READERS[n][1](g)
        except G.SvhError as e:
            raise AssertionError("%s keeps %s, yet the read launched a kernel (%s)" % (why, n, e))
        assert got == before[n], (why, n, "kept, but other bytes")
    G.lib().svh_test_fail_at(None)


def launches(G, g, n):
    """the read of output n needs a launch: it is not served from the cache"""
    G.lib().svh_test_fail_at(b"launch:1:0")
    try:
        TCC.READERS[n][1](g)
        out = False
    except G.SvhError:
        out = True
    G.lib().svh_test_fail_at(None)
    return out


@pytest.mark.parametrize("m", list(TCC.MUTATORS))
def test_matrix(G, hip, m):
    rig = TCC.Rig(G, hip)
    before = TCC.read_dev(rig.g)
    assert TCC.CC.REFUSED not in before.values()
    rig.apply(m)
    if m in TCC.LEFT_ALONE:
        served(G, rig.g, TCC.CACHED, before, m)
    if m in TCC.KEEPS_STATIC:
        served(G, rig.g, ["time:RCOST", "time:RPOT"], before, m)
        assert launches(G, rig.g, "time:TPOT"), m
    after = TCC.read_dev(rig.g)
    fresh = rig.fresh()
    assert TCC.read_dev(fresh) == after, "after %s a fresh object with the same history answers otherwise" % m
    fresh.close()
    rig.g.close()


def test_a_step_keeps_the_static_planes_without_release_and_drops_them_with_it(G, hip):
    for release in (0, 1):
        rig = TCC.Rig(G, hip)
        g = rig.g
        g.set_time(release=release)
        before = TCC.read_dev(g)
        assert (g.time_stats()[4] > 0) == (release == 1)
        OCC.objects_step(g, None, None)
        if release == 0:
            served(G, g, ["time:RCOST", "time:RPOT"], before, "objects_step with release = 0")
        else:
            assert launches(G, g, "time:RCOST"), "objects_step with release = 1 is to drop the static planes"
        assert launches(G, g, "time:TPOT"), "objects_step is to drop TPOT"
        g.close()


def test_the_first_entry_that_asks_computes_and_keeps(G, hip):
    for n in TCC.READERS:
        rig = TCC.Rig(G, hip)
        rig.apply("add_points")
        first = TCC.READERS[n][1](rig.g)
        if TCC.READERS[n][0] != "static":
            served(G, rig.g, TCC.CACHED, {k: TCC.READERS[k][1](rig.g) for k in TCC.CACHED}, "the first read of " + n)
        else:
            served(G, rig.g, ["time:RCOST", "time:RPOT"], {k: TCC.READERS[k][1](rig.g) for k in ("time:RCOST", "time:RPOT")}, "the first read of " + n)
        fresh = rig.fresh()
        assert TCC.READERS[n][1](fresh) == first, n
        fresh.close()
        rig.g.close()


def test_the_layer_leaves_the_other_layers_valid(G, hip):
    """the other way round: the layer's setter and reads drop no other layer's cache, the objects', the prediction's and the pose
    planner's included"""
    rig = TCC.Rig(G, hip)
    g = rig.g
    readers = {}
    for n, r in CC.READERS.items():
        if r.cached is True:
            try:
                r.dev(g)
                readers[n] = r.dev
            except G.SvhError:
                pass
    readers.update(("obj/" + n, OCC.READERS[n][1]) for n in OCC.CACHED)
    readers.update(("pred/" + n, PCC.READERS[n][1]) for n in PCC.CACHED)
    readers.update(("pose/" + n, QCC.READERS[n][1]) for n in QCC.CACHED)
    assert len(readers) > 20
    before = {n: f(g) for n, f in readers.items()}
    for m in TCC.OWN:
        TCC.OWN[m](g, None, None)
        TCC.read_dev(g)
    g.render_time(1)
    G.lib().svh_test_fail_at(b"launch:1:0")
    for n, f in readers.items():
        try:
            assert f(g) == before[n], n
        except G.SvhError as e:
            raise AssertionError("the time layer is to leave %s current, yet the read launched a kernel (%s)" % (n, e))
    G.lib().svh_test_fail_at(None)
    g.close()
