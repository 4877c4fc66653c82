"""GPU: the PRED bit of the engine's `valid` mask (stereo-vision_amd/csrc/grid_engine.cpp) pinned from outside, against the tables of
tests/grid_pred_cache_cases.py, which tests/test_grid_pred_cache.py pins on the CPU.

The rule under test is that of tests/test_grid_cache_gpu.py: a read through a cache is indistinguishable from a read computed from the
state as it is.  After every mutator of the grid -- those of every other layer and of the objects included -- and after the layer's
own, PRED, its statistics and a scored record are compared with the composed restatement and with a fresh object that replays the
history and is read once; an output that the documented rule keeps is served under the simulated error launch:1:0, that is without a
launch: no new computation.  Then the host-side failure hook in this layer's own entries: a failed allocation, launch, copy or wait
returns SVH_ERR_HIP, leaves the tracks, the grid and the other layers as they were, and the next call is correct.  Every comparison is
of bytes and exact.  The window is the scene's 33 x 17."""
import ctypes as C

import pytest

import grid_cache_cases as CC
import grid_obj_cache_cases as OCC
import grid_pred_cache_cases as PCC
import helpers as H   # puts the package on the path

pytestmark = pytest.mark.gpu
HIP_ERR = -2


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


@pytest.mark.parametrize("m", list(PCC.MUTATORS))
def test_matrix(G, hip, m):
    rig = PCC.Rig(G, hip)
    before = PCC.read_dev(rig.g)
    agree("the scene", before, PCC.read_ref(rig.ref))
    rig.apply(m)
    # KEEPS: the documented rule says PRED survives, so the plane and the statistics are served without a launch
    G.lib().svh_test_fail_at(b"launch:1:0")
    for n in PCC.CACHED:
        if PCC.served_from_cache(m, n):
            try:
                got = PCC.READERS[n][1](rig.g)
            except G.SvhError as e:
                raise AssertionError("%s keeps %s by the documented rule, yet the read launched a kernel (%s)" % (m, n, e))
            assert got == before[n], (m, n, "kept, but other bytes")
    G.lib().svh_test_fail_at(None)
    after = PCC.read_dev(rig.g)
    agree("after " + m, after, PCC.read_ref(rig.ref))
    fresh = rig.fresh()
    agree("after %s, a fresh object with the same history" % m, after, PCC.read_dev(fresh))
    fresh.close()
    for n in PCC.READERS:
        if PCC.EXPECT[m][n] == PCC.KEEPS:
            assert after[n] == before[n], (m, n, "the documented rule says this output stays")
        elif PCC.READERS[n][0] == "pred" and (m, n) not in PCC.UNSHOWN:
            assert after[n] != before[n], (m, n, "this output was to change")
    rig.g.close()


@pytest.mark.parametrize("n", list(PCC.READERS))
def test_the_first_entry_that_asks_computes_and_keeps(G, hip, n):
    """after a step PRED is stale and this entry is the first to find it so; afterwards the plane and the statistics are served without a
    launch"""
    rig = PCC.Rig(G, hip)
    rig.apply("objects_step")
    first = PCC.READERS[n][1](rig.g)
    G.lib().svh_test_fail_at(b"launch:1:0")
    try:
        kept = {k: PCC.READERS[k][1](rig.g) for k in PCC.CACHED}
    except G.SvhError as e:
        raise AssertionError("%s computed PRED and did not keep it: the next read launched a kernel (%s)" % (n, e))
    G.lib().svh_test_fail_at(None)
    want = PCC.read_ref(rig.ref)
    assert first == want[n] and all(kept[k] == want[k] for k in kept), n
    rig.g.close()


def test_the_prediction_leaves_the_other_layers_valid(G, hip):
    """the other way round: the layer's mutator and reads drop no other layer's cache, the objects' included"""
    rig = PCC.Rig(G, hip)
    before, obj_before = rig_read_all(rig), OCC.read_dev(rig.g)
    g = rig.g
    g.set_predict(G.default_pred(**PCC.OTHER_KW))
    PCC.read_dev(g)
    g.render_pred()
    g.footprint_pred(CC.POSES[:6])
    G.lib().svh_test_fail_at(b"launch:1:0")
    for n, r in CC.READERS.items():
        if r.cached is True and n in before:
            assert r.dev(g) == before[n], n
    for n in OCC.CACHED:
        assert OCC.READERS[n][1](g) == obj_before[n], n
    G.lib().svh_test_fail_at(None)
    assert OCC.read_dev(g) == obj_before
    g.close()


def rig_read_all(rig):
    out = {}
    for n, r in CC.READERS.items():
        if r.cached is True:
            try:
                out[n] = r.dev(rig.g)
            except rig.G.SvhError:
                pass
    return out


def snapshot(G, g):
    """the tracks, the objects and the grid's planes"""
    return dict(OCC.read_dev(g), count=g.count().tobytes(), hmax=g.hmax().tobytes(), cost=g.trav_plane(G.TRAV_COST).tobytes())


@pytest.mark.parametrize("spec", ["malloc:1", "launch:1", "copy:1", "copy:2", "wait:1"])
@pytest.mark.parametrize("n", list(PCC.READERS))
def test_a_failed_call_leaves_everything_else_and_the_next_is_correct(G, hip, n, spec):
    """a step makes PRED stale; the entry that finds it so fails at its first allocation, launch, copy or wait (a simulated error: nothing
    faults on the device)"""
    rig = PCC.Rig(G, hip)
    rig.apply("set_predict")                                      # the rows of the inflation are not allocated yet
    rig.apply("objects_step")
    if spec == "malloc:1":
        rig.g.set_predict(G.default_pred(**PCC.PRED_KW))           # this form needs them
        rig.ref.pred = PCC.PR.PredParams(**PCC.PRED_KW)
    before = snapshot(G, rig.g)
    G.lib().svh_test_fail_at(spec.encode())
    with pytest.raises(G.SvhError) as e:
        PCC.READERS[n][1](rig.g)
    G.lib().svh_test_fail_at(None)
    assert e.value.code == HIP_ERR, (n, spec, e.value.code)
    assert snapshot(G, rig.g) == before, (n, spec, "a failed call of the prediction changed the tracks, the objects or the grid")
    agree("the call repeated after %s" % spec, PCC.read_dev(rig.g), PCC.read_ref(rig.ref))
    rig.g.close()
