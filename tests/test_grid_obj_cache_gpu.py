"""GPU: the OBJ bit of the engine's `valid` mask and the state of the tracks (stereo-vision_amd/csrc/grid_engine.cpp) pinned from
outside, against the tables of tests/grid_obj_cache_cases.py, which tests/test_grid_obj_cache.py pins on the CPU.

The rule under test is that of tests/test_grid_cache_gpu.py: a read through a cache is indistinguishable from a read computed from the
state as it is.  After every mutator of the grid -- those of every other layer included -- and after the layer's own three, every
output of the object layer is compared with the composed restatement and with a fresh object that replays the history and is read
once; an output that the documented rule keeps is served under the simulated error launch:1:0, that is without a launch.  Every
comparison is of bytes and exact.  The window is the scene's 33 x 17."""
import ctypes as C

import pytest

import grid_cache_cases as CC
import grid_obj_cache_cases as OCC
import helpers as H   # puts the package on the path

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import svhip
    from svhip import grid
    assert svhip.device_count() > 0, "no HIP device: the product has no CPU fallback"
    svhip.lib().svh_test_fail_at.argtypes = [C.c_char_p]
    grid._bind()
    assert grid.FRONT_TILE == CC.T
    return grid


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


@pytest.fixture(autouse=True)
def restore(G):
    yield
    G.lib().svh_test_fail_at(None)


def agree(tag, dev, ref):
    bad = [n for n in dev if dev[n] != ref[n]]
    assert not bad, "%s: the object and the restatement differ on %s" % (tag, bad)


@pytest.mark.parametrize("m", list(OCC.MUTATORS))
def test_matrix(G, hip, m):
    rig = OCC.Rig(G, hip)
    before = OCC.read_dev(rig.g)
    agree("the scene", before, OCC.read_ref(rig.ref))
    rig.apply(m)
    # KEEPS: the documented rule says the cache survives, so the read is served without a launch
    G.lib().svh_test_fail_at(b"launch:1:0")
    for n, r in OCC.READERS.items():
        if OCC.served_from_cache(m, n) or r[0] == "tracks":       # the tracks are state: reading them never launches
            try:
                got = r[1](rig.g)
            except G.SvhError as e:
                raise AssertionError("%s keeps %s by the documented rule, yet the read launched a kernel (%s)" % (m, n, e))
            assert OCC.EXPECT[m][n] == OCC.CHANGES or got == before[n], (m, n, "kept, but other bytes")
    G.lib().svh_test_fail_at(None)
    after = OCC.read_dev(rig.g)
    agree("after " + m, after, OCC.read_ref(rig.ref))
    fresh = rig.fresh()
    agree("after %s, a fresh object with the same history" % m, after, OCC.read_dev(fresh))
    fresh.close()
    for n in OCC.READERS:
        if OCC.EXPECT[m][n] == OCC.KEEPS:
            assert after[n] == before[n], (m, n, "the documented rule says this output stays")
        elif (m, n) not in OCC.UNSHOWN:
            assert after[n] != before[n], (m, n, "this output was to change")
    # and a step from there: the tracks go on from what they were, on the object as on the restatement
    rig.apply("objects_step")
    agree("a step after " + m, OCC.read_dev(rig.g), OCC.read_ref(rig.ref))
    assert rig.g.last_assign.tolist() == rig.ref.last_assign.tolist()
    rig.g.close()


@pytest.mark.parametrize("n", OCC.CACHED)
def test_a_getter_keeps_what_it_computed(G, hip, n):
    """after a plain add the objects are stale and this getter is the first entry to find them so; the same read again is served
    without a launch"""
    rig = OCC.Rig(G, hip)
    rig.apply("add_points")
    first = OCC.READERS[n][1](rig.g)
    G.lib().svh_test_fail_at(b"launch:1:0")
    try:
        again = OCC.READERS[n][1](rig.g)
    except G.SvhError as e:
        raise AssertionError("%s computed the objects and did not keep them: the second read launched a kernel (%s)" % (n, e))
    G.lib().svh_test_fail_at(None)
    assert again == first == OCC.READERS[n][2](rig.ref), n
    rig.g.close()


def test_the_objects_leave_the_other_layers_valid(G, hip):
    """the other way round: the object layer's mutators and reads drop no other layer's cache"""
    rig = CC.Rig(G, hip)
    before = rig.read_all()
    g = rig.g
    g.set_objects(G.default_obj(**OCC.OBJ_KW))
    g.objects_step()
    g.obj_plane(G.OBJ_LABEL)
    g.render_objects()
    g.objects_reset()
    G.lib().svh_test_fail_at(b"launch:1:0")
    for n, r in CC.READERS.items():
        if r.cached is True:
            assert r.dev(g) == before[n][0], n
    G.lib().svh_test_fail_at(None)
    g.close()
