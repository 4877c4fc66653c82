"""GPU: the POSE_CF and POSE bits of the engine's `valid` mask (stereo-vision_amd/csrc/grid_engine.cpp) pinned from outside, against the
tables of tests/grid_pose_cache_cases.py, which tests/test_grid_pose_cache.py pins on the CPU.

The rule under test is that of tests/test_grid_cache_gpu.py: a read through a cache is indistinguishable from a read computed from the
state as it is.  After every mutator of the grid -- those of every other layer, of the objects and of the prediction included -- and
after the layer's own three, CF, PPOT, PDIR, the statistics and a path are compared with the composed restatement and with a fresh
object that replays the history and is read once; an output that the documented rule keeps is served under the simulated error
launch:1:0, that is without a launch: no new computation.  Every comparison is of bytes and exact.  The window is the scene's 33 x 17."""
import ctypes as C

import pytest

import grid_cache_cases as CC
import grid_obj_cache_cases as OCC
import grid_pose_cache_cases as QCC
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


@pytest.mark.parametrize("m", list(QCC.MUTATORS))
def test_matrix(G, hip, m):
    rig = QCC.Rig(G, hip)
    before = QCC.read_dev(rig.g)
    agree("the scene", before, QCC.read_ref(rig.ref))
    rig.apply(m)
    # KEEPS: the documented rule says the planes survive, so they and the statistics are served without a launch
    G.lib().svh_test_fail_at(b"launch:1:0")
    for n in QCC.CACHED:
        if QCC.served_from_cache(m, n):
            try:
                got = QCC.READERS[n][1](rig.g)
            except G.SvhError as e:
                raise AssertionError("%s keeps %s by the documented rule, yet the read launched a kernel (%s)" % (m, n, e))
            assert got == before[n], (m, n, "kept, but other bytes")
    G.lib().svh_test_fail_at(None)
    after = QCC.read_dev(rig.g)
    agree("after " + m, after, QCC.read_ref(rig.ref))
    fresh = rig.fresh()
    agree("after %s, a fresh object with the same history" % m, after, QCC.read_dev(fresh))
    fresh.close()
    for n in QCC.READERS:
        if QCC.EXPECT[m][n] == QCC.KEEPS:
            assert after[n] == before[n], (m, n, "the documented rule says this output stays")
        elif (m, n) not in QCC.UNSHOWN:
            assert after[n] != before[n], (m, n, "this output was to change")
    rig.g.close()


@pytest.mark.parametrize("n", list(QCC.READERS))
def test_the_first_entry_that_asks_computes_and_keeps(G, hip, n):
    """after an add the layer is stale and this entry is the first to find it so; afterwards the planes and the statistics are served
    without a launch.  CF alone does not compute the field: after it PPOT still needs its launches"""
    rig = QCC.Rig(G, hip)
    rig.apply("add_points")
    first = QCC.READERS[n][1](rig.g)
    G.lib().svh_test_fail_at(b"launch:1:0")
    kept = {}
    for k in QCC.CACHED:
        try:
            kept[k] = QCC.READERS[k][1](rig.g)
        except G.SvhError as e:
            assert n == "pose:CF" and k != "pose:CF", "%s computed the layer and did not keep %s: the next read launched a kernel (%s)" % (n, k, e)
    G.lib().svh_test_fail_at(None)
    want = QCC.read_ref(rig.ref)
    assert first == want[n] and all(kept[k] == want[k] for k in kept) and "pose:CF" in kept, n
    agree("afterwards", QCC.read_dev(rig.g), want)
    rig.g.close()


def test_the_layer_leaves_the_other_layers_valid(G, hip):
    """the other way round: the layer's mutators and reads drop no other layer's cache, the objects' and the prediction's included"""
    import grid_pred_cache_cases as PCC
    rig = QCC.Rig(G, hip)
    g = rig.g
    before = {n: r.dev(g) for n, r in CC.READERS.items() if r.cached is True and _reads(G, r, g)}
    obj_before, pred_before = OCC.read_dev(g), {n: PCC.READERS[n][1](g) for n in PCC.CACHED}
    for m in QCC.OWN:
        QCC.OWN[m](g, None, None)
        QCC.read_dev(g)
    g.render_pose()
    G.lib().svh_test_fail_at(b"launch:1:0")
    for n in before:
        assert CC.READERS[n].dev(g) == before[n], n
    for n in OCC.CACHED:
        assert OCC.READERS[n][1](g) == obj_before[n], n
    for n in PCC.CACHED:
        assert PCC.READERS[n][1](g) == pred_before[n], n
    G.lib().svh_test_fail_at(None)
    assert OCC.read_dev(g) == obj_before
    g.close()


def _reads(G, r, g):
    try:
        r.dev(g)
        return True
    except G.SvhError:
        return False
