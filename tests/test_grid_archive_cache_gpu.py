"""GPU: the archive and the engine's caches (stereo-vision_amd/csrc/grid_engine.cpp), on the scene and with the readers of
tests/grid_cache_cases.py, tests/grid_obj_cache_cases.py, tests/grid_pred_cache_cases.py and tests/grid_pose_cache_cases.py, which
this file imports and does not change.

The rule under test is that of tests/test_grid_cache_gpu.py: a read through a cache is indistinguishable from a read computed from the
state as it is.  Nothing cached is computed from the archive, so its mutators -- svh_grid_set_archive, svh_grid_archive_clear,
svh_grid_archive_trim -- leave every cached output current: it is served under the simulated error launch:1:0, that is without a
launch, with the bytes it had.  A scroll that restores cells drops what a scroll always dropped: afterwards every cached output
equals the one a fresh object computes that never scrolled, because the restored window is that object's window.  Every comparison is
of bytes and exact.  The window is the scene's 33 x 17."""
import ctypes as C

import pytest

import grid_cache_cases as CC
import grid_obj_cache_cases as OCC
import grid_pose_cache_cases as QCC
import grid_pred_cache_cases as PCC
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


def cached_readers(G, g):
    """name -> the read, for every output that is served from a cache on this scene"""
    out = {}
    for n, r in CC.READERS.items():
        if r.cached is True:
            try:
                r.dev(g)
                out[n] = r.dev
            except G.SvhError:
                pass
    out.update(("obj/" + n, OCC.READERS[n][1]) for n in OCC.CACHED)
    out.update(("pred/" + n, PCC.READERS[n][1]) for n in PCC.CACHED)
    out.update(("pose/" + n, QCC.READERS[n][1]) for n in QCC.CACHED)
    return out


def read(readers, g):
    return {n: f(g) for n, f in readers.items()}


MUTATORS = {
    "set_archive": lambda g: g.set_archive(max_tiles=32),
    "set_archive_same": lambda g: g.set_archive(max_tiles=64),
    "archive_trim": lambda g: g.archive_trim(0, 0, 5, 5),
    "archive_clear": lambda g: g.archive_clear(),
    "set_archive_off": lambda g: g.set_archive(max_tiles=0),
}


@pytest.mark.parametrize("m", list(MUTATORS))
def test_the_archive_mutators_leave_every_cache_current(G, hip, m):
    rig = QCC.Rig(G, hip)
    g = rig.g
    g.set_archive(max_tiles=64)
    g.scroll(5, 3)
    g.scroll(-5, -3)                                              # the archive holds tiles, the window is the scene's again
    assert g.archive_stats()["pages"] > 0 and g.archive_stats()["restored"] > 0
    readers = cached_readers(G, g)
    assert len(readers) > 20
    before = read(readers, g)
    MUTATORS[m](g)
    G.lib().svh_test_fail_at(b"launch:1:0")
    for n, f in readers.items():
        try:
            got = f(g)
        except G.SvhError as e:
            raise AssertionError("%s is to leave %s current, yet the read launched a kernel (%s)" % (m, n, e))
        assert got == before[n], (m, n, "kept, but other bytes")
    G.lib().svh_test_fail_at(None)
    g.close()


def test_a_scroll_that_restores_leaves_what_a_fresh_object_computes(G, hip):
    rig = QCC.Rig(G, hip)
    g = rig.g
    readers = cached_readers(G, g)
    before = read(readers, g)
    g.set_archive(max_tiles=64)
    g.scroll(5, 3)
    moved = read(readers, g)                                      # every cache is filled on the moved window
    assert any(moved[n] != before[n] for n in readers)
    g.scroll(-5, -3)
    st = g.archive_stats()
    assert st["restored"] > 0 and st["lost"] == 0
    after = read(readers, g)
    fresh = rig.fresh()                                           # the same history without a scroll, read once
    want = read(readers, fresh)
    bad = [n for n in readers if after[n] != want[n]]
    assert not bad, "after a scroll away and back these differ from a fresh object that never moved: %s" % bad
    assert [n for n in readers if after[n] != before[n]] == []
    fresh.close()
    g.close()
